"""Ellipsoidal map projections the engine supports, restated from PROJ.

The reference reaches these through pyproj/PROJ (``Transformer.from_crs``;
call sites reproject.py:124-126,347,398,483, rectify.py:196-203).  PROJ is
absent here, so the formulas PROJ uses are restated (radians in/out, unit
ellipsoid, ``a`` / false easting / northing applied by the caller exactly as
PROJ's ``pj_fwd`` / ``pj_inv`` do):

* ``TransverseMercator`` — PROJ ``tmerc`` with its default ``poder_engsager``
  algorithm (Krüger series to 6th order in n, Clenshaw summation: ``gatg``,
  ``clens``, ``clenS``), used for UTM zones (``+proj=utm``: k0 0.9996,
  central meridian 6*zone - 183, false easting 500 km, 10 000 km north offset
  for southern zones);
* ``LambertAzimuthalEqualArea`` — PROJ ``laea`` ellipsoidal oblique / equatorial
  / polar aspects (``pj_qsfn``, authalic latitude series ``pj_authset`` /
  ``pj_authlat``);
* ``PolarStereographic`` — PROJ ``stere`` in its two polar aspects on the
  ellipsoid (EPSG methods 9810 variant A: ``k0``, 9829 variant B: ``lat_ts``);
* ``LambertConformalConic`` — PROJ ``lcc`` on the ellipsoid, one or two standard
  parallels (EPSG methods 9801 / 9802; EPSG:3034, EPSG:2154);
* ``Geostationary`` — PROJ ``geos`` on the ellipsoid, both sweep axes (CF
  ``geostationary``);
* ``AlbersEqualArea`` — PROJ ``aea`` on the ellipsoid, one or two standard
  parallels, either hemisphere (EPSG:5070, 3577, 3005; CF
  ``albers_conical_equal_area``);
* ``Sinusoidal`` — PROJ ``sinu`` on the ellipsoid, the sphere as its es = 0 case
  (the MODIS / VIIRS land grid; CF ``sinusoidal``);
* ``RotatedPole`` — PROJ ``ob_tran +o_proj=longlat`` as CF's
  ``rotated_latitude_longitude`` defines it (degrees on both sides).

Parity: PROJ's results are not available here; the restatement is pinned by
the reference's own PROJ-dependent test goldens (tests/test_reproject.py,
tests/test_spatial.py, tests/test_rectify.py) that the GPU tests check.
All functions are vectorised numpy, float64.
"""

from __future__ import annotations

import math

import numpy as np

_ORDER = 6  # PROJ_ETMERC_ORDER


class Ellipsoid:
    def __init__(self, name: str, a: float, rf: float):
        self.name = name
        self.a = a
        self.rf = rf
        f = 1.0 / rf
        self.f = f
        self.es = 2.0 * f - f * f
        self.e = math.sqrt(self.es)
        self.one_es = 1.0 - self.es
        self.b = a * (1.0 - f)


WGS84 = Ellipsoid("WGS 84", 6378137.0, 298.257223563)
GRS80 = Ellipsoid("GRS 1980", 6378137.0, 298.257222101)


# ---- Clenshaw summations (PROJ tmerc.cpp) -----------------------------------
def _gatg(p, B, cos_2B, sin_2B):
    two_cos_2B = 2.0 * cos_2B
    h2 = 0.0
    h1 = p[-1]
    h = 0.0
    for coef in p[-2::-1]:
        h = -h2 + two_cos_2B * h1 + coef
        h2 = h1
        h1 = h
    return B + h * sin_2B


def _clens(a, arg_r):
    r = 2.0 * math.cos(arg_r)
    hr1 = 0.0
    hr = a[-1]
    for coef in a[-2::-1]:
        hr2 = hr1
        hr1 = hr
        hr = -hr2 + r * hr1 + coef
    return math.sin(arg_r) * hr


def _clenS(a, sin_arg_r, cos_arg_r, sinh_arg_i, cosh_arg_i):
    r = 2.0 * cos_arg_r * cosh_arg_i
    i = -2.0 * sin_arg_r * sinh_arg_i
    hi1 = hr1 = hi = 0.0
    hr = a[-1]
    for coef in a[-2::-1]:
        hr2 = hr1
        hi2 = hi1
        hr1 = hr
        hi1 = hi
        hr = -hr2 + r * hr1 - i * hi1 + coef
        hi = -hi2 + i * hr1 + r * hi1
    r = sin_arg_r * cosh_arg_i
    i = cos_arg_r * sinh_arg_i
    return r * hr - i * hi, r * hi + i * hr


class TransverseMercator:
    """PROJ tmerc, algo poder_engsager (tmerc.cpp setup_exact / exact_e_fwd /
    exact_e_inv).  lam/phi in radians relative to the central meridian."""

    def __init__(self, ell: Ellipsoid, k0: float, phi0: float = 0.0):
        self.ell = ell
        es = ell.es
        f = es / (1.0 + math.sqrt(1.0 - es))
        n = f / (2.0 - f)
        np_ = n
        cgb = [0.0] * _ORDER
        cbg = [0.0] * _ORDER
        utg = [0.0] * _ORDER
        gtu = [0.0] * _ORDER
        cgb[0] = n * (2 + n * (-2 / 3.0 + n * (-2 + n * (116 / 45.0 + n * (26 / 45.0 + n * (-2854 / 675.0))))))
        cbg[0] = n * (-2 + n * (2 / 3.0 + n * (4 / 3.0 + n * (-82 / 45.0 + n * (32 / 45.0 + n * (4642 / 4725.0))))))
        np_ = n * n
        cgb[1] = np_ * (7 / 3.0 + n * (-8 / 5.0 + n * (-227 / 45.0 + n * (2704 / 315.0 + n * (2323 / 945.0)))))
        cbg[1] = np_ * (5 / 3.0 + n * (-16 / 15.0 + n * (-13 / 9.0 + n * (904 / 315.0 + n * (-1522 / 945.0)))))
        np_ *= n
        cgb[2] = np_ * (56 / 15.0 + n * (-136 / 35.0 + n * (-1262 / 105.0 + n * (73814 / 2835.0))))
        cbg[2] = np_ * (-26 / 15.0 + n * (34 / 21.0 + n * (8 / 5.0 + n * (-12686 / 2835.0))))
        np_ *= n
        cgb[3] = np_ * (4279 / 630.0 + n * (-332 / 35.0 + n * (-399572 / 14175.0)))
        cbg[3] = np_ * (1237 / 630.0 + n * (-12 / 5.0 + n * (-24832 / 14175.0)))
        np_ *= n
        cgb[4] = np_ * (4174 / 315.0 + n * (-144838 / 6237.0))
        cbg[4] = np_ * (-734 / 315.0 + n * (109598 / 31185.0))
        np_ *= n
        cgb[5] = np_ * (601676 / 22275.0)
        cbg[5] = np_ * (444337 / 155925.0)
        np_ = n * n
        self.Qn = k0 / (1 + n) * (1 + np_ * (1 / 4.0 + np_ * (1 / 64.0 + np_ / 256.0)))
        utg[0] = n * (-0.5 + n * (2 / 3.0 + n * (-37 / 96.0 + n * (1 / 360.0 + n * (81 / 512.0 + n * (-96199 / 604800.0))))))
        gtu[0] = n * (0.5 + n * (-2 / 3.0 + n * (5 / 16.0 + n * (41 / 180.0 + n * (-127 / 288.0 + n * (7891 / 37800.0))))))
        utg[1] = np_ * (-1 / 48.0 + n * (-1 / 15.0 + n * (437 / 1440.0 + n * (-46 / 105.0 + n * (1118711 / 3870720.0)))))
        gtu[1] = np_ * (13 / 48.0 + n * (-3 / 5.0 + n * (557 / 1440.0 + n * (281 / 630.0 + n * (-1983433 / 1935360.0)))))
        np_ *= n
        utg[2] = np_ * (-17 / 480.0 + n * (37 / 840.0 + n * (209 / 4480.0 + n * (-5569 / 90720.0))))
        gtu[2] = np_ * (61 / 240.0 + n * (-103 / 140.0 + n * (15061 / 26880.0 + n * (167603 / 181440.0))))
        np_ *= n
        utg[3] = np_ * (-4397 / 161280.0 + n * (11 / 504.0 + n * (830251 / 7257600.0)))
        gtu[3] = np_ * (49561 / 161280.0 + n * (-179 / 168.0 + n * (6601661 / 7257600.0)))
        np_ *= n
        utg[4] = np_ * (-4583 / 161280.0 + n * (108847 / 3991680.0))
        gtu[4] = np_ * (34729 / 80640.0 + n * (-3418889 / 1995840.0))
        np_ *= n
        utg[5] = np_ * (-20648693 / 638668800.0)
        gtu[5] = np_ * (212378941 / 319334400.0)
        self.cgb, self.cbg, self.utg, self.gtu = cgb, cbg, utg, gtu
        Z = _gatg(cbg, phi0, math.cos(2 * phi0), math.sin(2 * phi0))
        self.Zb = -self.Qn * (Z + _clens(gtu, 2 * Z))

    def forward(self, lam, phi):
        lam = np.asarray(lam, dtype=np.float64)
        phi = np.asarray(phi, dtype=np.float64)
        Cn = _gatg(self.cbg, phi, np.cos(2 * phi), np.sin(2 * phi))
        sin_Cn, cos_Cn = np.sin(Cn), np.cos(Cn)
        sin_Ce, cos_Ce = np.sin(lam), np.cos(lam)
        cos_Cn_cos_Ce = cos_Cn * cos_Ce
        Cn = np.arctan2(sin_Cn, cos_Cn_cos_Ce)
        inv_denom_tan_Ce = 1.0 / np.hypot(sin_Cn, cos_Cn_cos_Ce)
        tan_Ce = sin_Ce * cos_Cn * inv_denom_tan_Ce
        Ce = np.arcsinh(tan_Ce)
        two_inv_denom_tan_Ce = 2 * inv_denom_tan_Ce
        two_inv_denom_tan_Ce_square = two_inv_denom_tan_Ce * inv_denom_tan_Ce
        tmp_r = cos_Cn_cos_Ce * two_inv_denom_tan_Ce_square
        sin_arg_r = sin_Cn * tmp_r
        cos_arg_r = cos_Cn_cos_Ce * tmp_r - 1
        sinh_arg_i = tan_Ce * two_inv_denom_tan_Ce
        cosh_arg_i = two_inv_denom_tan_Ce_square - 1
        dCn, dCe = _clenS(self.gtu, sin_arg_r, cos_arg_r, sinh_arg_i, cosh_arg_i)
        Cn = Cn + dCn
        Ce = Ce + dCe
        ok = np.abs(Ce) <= 2.623395162778
        x = np.where(ok, self.Qn * Ce, np.inf)
        y = np.where(ok, self.Qn * Cn + self.Zb, np.inf)
        return x, y

    def inverse(self, x, y):
        x = np.asarray(x, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        Cn = (y - self.Zb) / self.Qn
        Ce = x / self.Qn
        ok = np.abs(Ce) <= 2.623395162778
        sin_arg_r = np.sin(2 * Cn)
        cos_arg_r = np.cos(2 * Cn)
        exp_2_Ce = np.exp(2 * Ce)
        half_inv_exp_2_Ce = 0.5 / exp_2_Ce
        sinh_arg_i = 0.5 * exp_2_Ce - half_inv_exp_2_Ce
        cosh_arg_i = 0.5 * exp_2_Ce + half_inv_exp_2_Ce
        dCn, dCe = _clenS(self.utg, sin_arg_r, cos_arg_r, sinh_arg_i, cosh_arg_i)
        Cn = Cn + dCn
        Ce = Ce + dCe
        sin_Cn, cos_Cn = np.sin(Cn), np.cos(Cn)
        sinhCe = np.sinh(Ce)
        Ce = np.arctan2(sinhCe, cos_Cn)
        modulus_Ce = np.hypot(sinhCe, cos_Cn)
        Cn = np.arctan2(sin_Cn, modulus_Ce)
        tmp = 2 * modulus_Ce / (sinhCe * sinhCe + 1)
        sin_2_Cn = sin_Cn * tmp
        cos_2_Cn = tmp * modulus_Ce - 1.0
        phi = _gatg(self.cgb, Cn, cos_2_Cn, sin_2_Cn)
        return np.where(ok, Ce, np.inf), np.where(ok, phi, np.inf)


# ---- Lambert azimuthal equal area (PROJ laea.cpp) ------------------------------
_EPS10 = 1.0e-10
_P00, _P01, _P02 = 0.33333333333333333333, 0.17222222222222222222, 0.10257936507936507937
_P10, _P11, _P20 = 0.06388888888888888888, 0.06640211640211640212, 0.01677689594356261023


def _qsfn(sinphi, e, one_es):
    con = e * sinphi
    div1 = 1.0 - con * con
    div2 = 1.0 + con
    return one_es * (sinphi / div1 - (0.5 / e) * np.log((1.0 - con) / div2))


class LambertAzimuthalEqualArea:
    """PROJ laea, ellipsoidal (e_forward / e_inverse)."""

    def __init__(self, ell: Ellipsoid, phi0: float):
        self.ell = ell
        self.phi0 = phi0
        e, es, one_es = ell.e, ell.es, ell.one_es
        t = abs(phi0)
        if abs(t - math.pi / 2) < _EPS10:
            self.mode = "npole" if phi0 >= 0 else "spole"
        elif abs(t) < _EPS10:
            self.mode = "equit"
        else:
            self.mode = "obliq"
        self.qp = float(_qsfn(1.0, e, one_es))
        self.mmf = 0.5 / (1.0 - es)
        t2 = es * es
        self.apa = (es * _P00 + t2 * _P01 + t2 * es * _P02, t2 * _P10 + t2 * es * _P11,
                    t2 * es * _P20)
        if self.mode in ("npole", "spole"):
            self.dd = 1.0
        elif self.mode == "equit":
            self.rq = math.sqrt(0.5 * self.qp)
            self.dd = 1.0 / self.rq
            self.xmf = 1.0
            self.ymf = 0.5 * self.qp
        else:
            self.rq = math.sqrt(0.5 * self.qp)
            sinphi = math.sin(phi0)
            self.sinb1 = float(_qsfn(sinphi, e, one_es)) / self.qp
            self.cosb1 = math.sqrt(1.0 - self.sinb1 * self.sinb1)
            self.dd = math.cos(phi0) / (math.sqrt(1.0 - es * sinphi * sinphi) * self.rq *
                                        self.cosb1)
            self.ymf = self.rq / self.dd
            self.xmf = self.rq * self.dd

    def _authlat(self, beta):
        t = beta + beta
        a = self.apa
        return beta + a[0] * np.sin(t) + a[1] * np.sin(t + t) + a[2] * np.sin(t + t + t)

    def forward(self, lam, phi):
        lam = np.asarray(lam, dtype=np.float64)
        phi = np.asarray(phi, dtype=np.float64)
        e, one_es = self.ell.e, self.ell.one_es
        coslam, sinlam, sinphi = np.cos(lam), np.sin(lam), np.sin(phi)
        q = _qsfn(sinphi, e, one_es)
        if self.mode in ("obliq", "equit"):
            sinb = q / self.qp
            cosb2 = 1.0 - sinb * sinb
            cosb = np.where(cosb2 > 0, np.sqrt(np.maximum(cosb2, 0.0)), 0.0)
            if self.mode == "obliq":
                b = 1.0 + self.sinb1 * sinb + self.cosb1 * cosb * coslam
            else:
                b = 1.0 + cosb * coslam
            bad = np.abs(b) < _EPS10
            b = np.sqrt(2.0 / np.where(bad, 1.0, b))
            if self.mode == "obliq":
                y = self.ymf * b * (self.cosb1 * sinb - self.sinb1 * cosb * coslam)
            else:
                y = b * sinb * self.ymf
            x = self.xmf * b * cosb * sinlam
            return np.where(bad, np.inf, x), np.where(bad, np.inf, y)
        q = self.qp - q if self.mode == "npole" else self.qp + q
        pos = q >= 1e-15
        b = np.sqrt(np.where(pos, q, 0.0))
        x = np.where(pos, b * sinlam, 0.0)
        y = np.where(pos, coslam * (b if self.phi0 < 0.0 else -b), 0.0)
        return x, y

    def inverse(self, x, y):
        x = np.asarray(x, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        if self.mode in ("obliq", "equit"):
            x = x / self.dd
            y = y * self.dd
            rho = np.hypot(x, y)
            small = rho < _EPS10
            rho_s = np.where(small, 1.0, rho)
            asin_arg = 0.5 * rho_s / self.rq
            bad = asin_arg > 1.0
            sCe = 2.0 * np.arcsin(np.minimum(asin_arg, 1.0))
            cCe = np.cos(sCe)
            sCe = np.sin(sCe)
            x = x * sCe
            if self.mode == "obliq":
                ab = cCe * self.sinb1 + y * sCe * self.cosb1 / rho_s
                y = rho_s * self.cosb1 * cCe - y * self.sinb1 * sCe
            else:
                ab = y * sCe / rho_s
                y = rho_s * cCe
            lam = np.arctan2(x, y)
            phi = self._authlat(np.arcsin(np.clip(ab, -1.0, 1.0)))
            lam = np.where(small, 0.0, lam)
            phi = np.where(small, self.phi0, phi)
            return np.where(bad, np.inf, lam), np.where(bad, np.inf, phi)
        if self.mode == "npole":
            y = -y
        q = x * x + y * y
        ab = 1.0 - q / self.qp
        if self.mode == "spole":
            ab = -ab
        lam = np.arctan2(x, y)
        phi = self._authlat(np.arcsin(np.clip(ab, -1.0, 1.0)))
        return lam, phi


# ---- Polar stereographic (PROJ stere.cpp, N_POLE / S_POLE on the ellipsoid) ------
_HALFPI = 0.5 * math.pi


def _tsfn(sinphi, cosphi, e):
    """PROJ pj_tsfn without pow: tan(pi/4 - phi/2) ((1 + e sin phi) / (1 - e sin
    phi))^(e/2), the power as exp(e atanh(e sin phi)) with atanh through one
    log, the tangent in the half-angle form that keeps its relative accuracy
    towards the pole."""
    con = e * sinphi
    with np.errstate(divide="ignore", invalid="ignore"):
        half = np.where(sinphi > 0, cosphi / (1.0 + sinphi), (1.0 - sinphi) / cosphi)
    return np.exp(e * (0.5 * np.log((1.0 + con) / (1.0 - con)))) * half


class PolarStereographic:
    """PROJ stere, ellipsoidal, |lat_0| = 90 deg (e_forward / e_inverse, N_POLE
    and S_POLE).  ``phits`` (variant B, radians) or, when it is None, ``k0``
    (variant A).  The inverse is the conformal -> geodetic latitude series
    (tmerc's ``cgb`` through ``_gatg``) applied to chi = pi/2 - 2 atan(t), whose
    sine and cosine are rational in t, instead of PROJ's data-dependent
    iteration."""

    def __init__(self, ell: Ellipsoid, phi0: float, phits: float | None, k0: float = 1.0):
        if abs(abs(phi0) - _HALFPI) >= _EPS10:
            raise ValueError("PolarStereographic needs lat_0 = +-90 degrees")
        self.ell = ell
        self.south = phi0 < 0
        e = ell.e
        phits = _HALFPI if phits is None else abs(phits)
        if abs(phits - _HALFPI) < _EPS10:
            self.akm1 = 2.0 * k0 / math.sqrt(math.pow(1 + e, 1 + e) * math.pow(1 - e, 1 - e))
        else:
            t = math.sin(phits)
            self.akm1 = (math.cos(phits) / float(_tsfn(t, math.cos(phits), e))
                         / math.sqrt(1.0 - (e * t) * (e * t)))
        self.cgb = TransverseMercator(ell, 1.0).cgb

    def forward(self, lam, phi):
        lam = np.asarray(lam, dtype=np.float64)
        phi = np.asarray(phi, dtype=np.float64)
        if self.south:
            phi = -phi
        sinlam, coslam = np.sin(lam), np.cos(lam)
        sinphi, cosphi = np.sin(phi), np.cos(phi)
        rho = self.akm1 * _tsfn(sinphi, cosphi, self.ell.e)
        rho = np.where(np.abs(phi - _HALFPI) < 1e-15, 0.0, rho)
        rho = np.where(phi + _HALFPI < _EPS10, np.inf, rho)   # the opposite pole
        x = rho * sinlam
        y = rho * coslam if self.south else -rho * coslam
        return x, y

    def inverse(self, x, y):
        x = np.asarray(x, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        if not self.south:
            y = -y
        t = np.sqrt(x * x + y * y) / self.akm1   # a few earth radii at most: no scaling
        t2 = t * t
        den = 1.0 + t2
        with np.errstate(invalid="ignore"):
            sin_chi = (1.0 - t2) / den
            cos_chi = (t + t) / den
        chi = _HALFPI - 2.0 * np.arctan(t)
        sin_2chi = 2.0 * sin_chi * cos_chi
        cos_2chi = (cos_chi - sin_chi) * (cos_chi + sin_chi)
        phi = _gatg(self.cgb, chi, cos_2chi, sin_2chi)
        lam = np.where((x == 0.0) & (y == 0.0), 0.0, np.arctan2(x, y))
        return lam, (-phi if self.south else phi)


# ---- Lambert conformal conic (PROJ lcc.cpp on the ellipsoid, 1SP and 2SP) ----------
def _msfn(sinphi, cosphi, es):
    return cosphi / math.sqrt(1.0 - es * sinphi * sinphi)


class LambertConformalConic:
    """PROJ lcc, ellipsoidal (lcc_e_forward / lcc_e_inverse).  ``phi1 == phi2``
    is the 1SP form; n < 0 puts the cone's apex over the south pole (c < 0
    then).  The power is exp(n log ts); the inverse takes the latitude from
    ts = (rho / c)^(1/n) by the series PolarStereographic.inverse uses, in
    place of PROJ's ``pj_phi2`` iteration."""

    def __init__(self, ell: Ellipsoid, phi0: float, phi1: float, phi2: float, k0: float = 1.0):
        if abs(phi1 + phi2) < _EPS10:
            raise ValueError("LambertConformalConic: lat_1 = -lat_2 is no cone")
        self.ell = ell
        self.k0 = k0
        e, es = ell.e, ell.es
        sinphi, cosphi = math.sin(phi1), math.cos(phi1)
        n = sinphi
        m1 = _msfn(sinphi, cosphi, es)
        ml1 = float(_tsfn(sinphi, cosphi, e))
        if abs(phi1 - phi2) >= _EPS10:   # secant cone
            sinphi, cosphi = math.sin(phi2), math.cos(phi2)
            n = math.log(m1 / _msfn(sinphi, cosphi, es))
            n /= math.log(ml1 / float(_tsfn(sinphi, cosphi, e)))
        self.n = n
        self.c = m1 * math.pow(ml1, -n) / n
        self.rho0 = 0.0 if abs(abs(phi0) - _HALFPI) < _EPS10 else \
            self.c * math.pow(float(_tsfn(math.sin(phi0), math.cos(phi0), e)), n)
        self.cgb = TransverseMercator(ell, 1.0).cgb

    def forward(self, lam, phi):
        lam = np.asarray(lam, dtype=np.float64)
        phi = np.asarray(phi, dtype=np.float64)
        n = self.n
        sinphi, cosphi = np.sin(phi), np.cos(phi)
        with np.errstate(divide="ignore", invalid="ignore"):
            rho = self.c * np.exp(n * np.log(_tsfn(sinphi, cosphi, self.ell.e)))
        pole = np.abs(np.abs(phi) - _HALFPI) < _EPS10
        bad = pole & (phi * n <= 0.0)   # the pole opposite the apex
        rho = np.where(pole, 0.0, rho)
        sinl, cosl = np.sin(n * lam), np.cos(n * lam)
        x = self.k0 * (rho * sinl)
        y = self.k0 * (self.rho0 - rho * cosl)
        return np.where(bad, np.inf, x), np.where(bad, np.inf, y)

    def inverse(self, x, y):
        n = self.n
        x = np.asarray(x, dtype=np.float64) / self.k0
        y = self.rho0 - np.asarray(y, dtype=np.float64) / self.k0
        rho = np.sqrt(x * x + y * y)   # a few earth radii at most: no scaling
        apex = rho == 0.0
        if n < 0.0:
            rho, x, y = -rho, -x, -y
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.exp(np.log(rho / self.c) * (1.0 / n))
            t2 = t * t
            den = 1.0 + t2
            sin_chi = (1.0 - t2) / den
            cos_chi = (t + t) / den
            chi = _HALFPI - 2.0 * np.arctan(t)
            sin_2chi = 2.0 * sin_chi * cos_chi
            cos_2chi = (cos_chi - sin_chi) * (cos_chi + sin_chi)
            phi = _gatg(self.cgb, chi, cos_2chi, sin_2chi)
            lam = np.where(apex, 0.0, np.arctan2(x, y) / n)
        return lam, np.where(apex, -_HALFPI if n < 0.0 else _HALFPI, phi)


# ---- Geostationary satellite view (PROJ geos.cpp on the ellipsoid) -----------------
class Geostationary:
    """PROJ geos, ellipsoidal (e_forward / e_inverse), ``h`` the perspective point
    height in metres, ``sweep`` "y" (PROJ's default: Meteosat, Himawari) or "x"
    (GOES).  Coordinates are scan angles times h / a on the unit ellipsoid.  The
    operations are the device's (xrs_proj.hpp geos_fwd / geos_inv): PROJ's
    geocentric latitude and radius folded into w = 1 / sqrt(cos^2 + (1 - es)
    sin^2), the arctangents of quotients as arctan2 (their second arguments are
    positive).  Where the satellite does not see the point (forward) or the ray
    passes the limb (inverse) both results are +inf."""

    def __init__(self, ell: Ellipsoid, h: float, sweep: str = "y"):
        if sweep not in ("x", "y"):
            raise ValueError(f"geos sweep axis must be 'x' or 'y', was {sweep!r}")
        self.ell = ell
        self.flip = sweep == "x"
        self.radius_g_1 = h / ell.a
        self.radius_g = 1.0 + self.radius_g_1
        self.C = self.radius_g * self.radius_g - 1.0
        self.radius_p = math.sqrt(ell.one_es)
        self.radius_p_inv2 = 1.0 / ell.one_es

    def forward(self, lam, phi):
        lam = np.asarray(lam, dtype=np.float64)
        phi = np.asarray(phi, dtype=np.float64)
        sinlam, coslam = np.sin(lam), np.cos(lam)
        sinphi, cosphi = np.sin(phi), np.cos(phi)
        pz = self.ell.one_es * sinphi
        w = 1.0 / np.sqrt(cosphi * cosphi + pz * sinphi)
        r = w * cosphi
        Vx, Vy, Vz = r * coslam, r * sinlam, w * pz
        tmp = self.radius_g - Vx
        with np.errstate(invalid="ignore"):
            bad = (tmp * Vx - Vy * Vy - Vz * Vz * self.radius_p_inv2) < 0.0
        other = Vz if self.flip else Vy
        h = np.sqrt(other * other + tmp * tmp)
        ax = np.arctan2(Vy, h if self.flip else tmp)
        ay = np.arctan2(Vz, tmp if self.flip else h)
        return (np.where(bad, np.inf, self.radius_g_1 * ax),
                np.where(bad, np.inf, self.radius_g_1 * ay))

    def inverse(self, x, y):
        x = np.asarray(x, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        tx, ty = np.tan(x / self.radius_g_1), np.tan(y / self.radius_g_1)
        first = ty if self.flip else tx
        stretch = np.sqrt(1.0 + first * first)
        Vy = tx * stretch if self.flip else tx
        Vz = ty if self.flip else ty * stretch
        zp = Vz / self.radius_p
        q = Vy * Vy + zp * zp
        # a quarter of PROJ's b^2 - 4 a C (a = 1 + q), without its cancellation
        det = 1.0 - q * self.C
        with np.errstate(invalid="ignore"):
            bad = det < 0.0
        k = (self.radius_g - np.sqrt(np.where(bad, 0.0, det))) / (1.0 + q)
        Vx = self.radius_g - k
        Vy = Vy * k
        Vz = Vz * k
        lam = np.arctan2(Vy, Vx)
        phi = np.arctan2(self.radius_p_inv2 * Vz, np.sqrt(Vx * Vx + Vy * Vy))
        return np.where(bad, np.inf, lam), np.where(bad, np.inf, phi)


# ---- Albers equal-area conic (PROJ aea.cpp on the ellipsoid) ------------------------
_TOL7 = 1.0e-7


def _qsfn_atanh(sinphi, e, one_es):
    """pj_qsfn with the logarithm as atanh(e sin phi): ``_qsfn``'s log of a quotient
    near 1 carries an absolute error of an ulp of 1, which its factor 0.5 / e = 6
    makes 6e-16 of q; that is 2e-15 of the cone constant n and 3e-8 m at the far
    pole.  laea keeps ``_qsfn`` (its results are pinned); aea uses this one."""
    con = e * sinphi
    return one_es * (sinphi / (1.0 - con * con) + np.arctanh(con) / e)


def _sine_series(fn, order: int = _ORDER, samples: int = 32):
    """The first ``order`` coefficients of the odd, pi-periodic ``fn`` as a series
    sum_j A_j sin(2 j t), by the midpoint sine transform over (0, pi/2).  The
    auxiliary-latitude differences have coefficients of size n^j, so aliasing
    (from j = 2 samples -+ j on) and the truncation lie below 1e-20."""
    t = (np.arange(samples) + 0.5) * (_HALFPI / samples)
    g = fn(t)
    return [float(2.0 / samples * np.sum(g * np.sin(2 * j * t))) for j in range(1, order + 1)]


def _authalic_to_geodetic(ell: Ellipsoid):
    """phi - beta = sum_j A_j sin(2 j beta), j = 1..6: the authalic -> geodetic
    latitude series, its coefficients taken numerically per ellipsoid (Newton on
    q(phi) = qp sin beta, Snyder (3-16), run to convergence at the sample points
    when the CRS is made, never per point)."""
    e, es, one_es = ell.e, ell.es, ell.one_es
    qp = float(_qsfn_atanh(1.0, e, one_es))

    def diff(beta):
        q, phi = qp * np.sin(beta), beta.copy()
        for _ in range(8):   # quadratic from an error of es / 3: exact after 4
            s = np.sin(phi)
            con = 1.0 - es * s * s
            phi = phi + con * con / (2.0 * np.cos(phi)) * ((q - _qsfn_atanh(s, e, one_es)) / one_es)
        return phi - beta

    return _sine_series(diff)


class AlbersEqualArea:
    """PROJ aea, ellipsoidal (aea.cpp e_forward / e_inverse).  ``phi1 == phi2`` is
    the one-parallel form; n < 0 puts the apex over the south pole.  The inverse
    takes the latitude from q = (c - (rho n)^2) / n through the authalic latitude
    beta (sin beta = q / qp) and a 6-term sine series in 2 beta (``apa``), in place of
    PROJ's ``phi1_`` iteration; |q| within PROJ's 1e-7 of qp is the pole, |q|
    beyond that is outside the projection: both results +inf."""

    def __init__(self, ell: Ellipsoid, phi0: float, phi1: float, phi2: float):
        if abs(phi1 + phi2) < _EPS10:
            raise ValueError("AlbersEqualArea: lat_1 = -lat_2 is no cone")
        self.ell = ell
        # The constants are PROJ's, taken in extended precision and rounded once: n is
        # a quotient of two differences (m1^2 - m2^2 and q2 - q1 cancel a digit each), and
        # in float64 its error of 1e-15 is 2e-8 m at the far pole and 2e-12 deg in the
        # inverse next to a pole, where q is flat.  (Where long double is float64 the
        # constants are merely float64's.)
        ld = np.longdouble
        es = ld(ell.es)
        e, one_es = np.sqrt(es), 1.0 - es

        def msq(phi):   # pj_msfn squared
            return np.cos(ld(phi)) ** 2 / (1.0 - es * np.sin(ld(phi)) ** 2)

        def qs(phi):
            return _qsfn_atanh(np.sin(ld(phi)), e, one_es)

        n, ml1 = np.sin(ld(phi1)), qs(phi1)
        if abs(phi1 - phi2) >= _EPS10:   # secant cone
            n = (msq(phi1) - msq(phi2)) / (qs(phi2) - ml1)
        c = msq(phi1) + n * ml1
        self.n, self.dd, self.n2, self.c = float(n), float(1.0 / n), float(n * n), float(c)
        self.qp = float(qs(_HALFPI))                    # PROJ's ec
        self.rho0 = float(np.sqrt(c - n * qs(phi0)) / n)
        self.apa = _authalic_to_geodetic(ell)

    def forward(self, lam, phi):
        lam = np.asarray(lam, dtype=np.float64)
        phi = np.asarray(phi, dtype=np.float64)
        rad = self.c - self.n * _qsfn_atanh(np.sin(phi), self.ell.e, self.ell.one_es)
        with np.errstate(invalid="ignore"):
            bad = rad < 0.0
        rho = self.dd * np.sqrt(np.where(bad, 0.0, rad))
        nl = self.n * lam
        x = rho * np.sin(nl)
        y = self.rho0 - rho * np.cos(nl)
        return np.where(bad, np.inf, x), np.where(bad, np.inf, y)

    def inverse(self, x, y):
        n = self.n
        x = np.asarray(x, dtype=np.float64)
        y = self.rho0 - np.asarray(y, dtype=np.float64)
        r2 = x * x + y * y             # a few earth radii at most: no scaling
        apex = r2 == 0.0
        if n < 0.0:
            x, y = -x, -y
        q = (self.c - self.n2 * r2) / n   # rho only through its square: no sqrt
        with np.errstate(invalid="ignore"):
            pole = np.abs(self.qp - np.abs(q)) <= _TOL7
            bad = ~pole & ~apex & (np.abs(q) > self.qp)
            sb = np.clip(q / self.qp, -1.0, 1.0)
            cb = np.sqrt((1.0 - sb) * (1.0 + sb))
            phi = _gatg(self.apa, np.arcsin(sb), (cb - sb) * (cb + sb), 2.0 * sb * cb)
            phi = np.where(pole, np.copysign(_HALFPI, q), phi)
            lam = np.where(apex, 0.0, np.arctan2(x, y) * self.dd)
        phi = np.where(apex, -_HALFPI if n < 0.0 else _HALFPI, phi)
        return np.where(bad, np.inf, lam), np.where(bad, np.inf, phi)


# ---- Sinusoidal (PROJ gn_sinu.cpp sinu on the ellipsoid; the sphere is es = 0) -------
def _rectifying_series(ell: Ellipsoid):
    """(cmu, cphi): mu - phi = sum_j cmu_j sin(2 j phi) and phi - mu = sum_j cphi_j
    sin(2 j mu), j = 1..6, the geodetic <-> rectifying latitude series in the third
    flattening n (Karney 2011, eqs. 35-36 extended to n^6).  The meridian arc from
    the equator is M(phi) = Qn mu with tmerc's Qn at k0 = 1; at es = 0 every
    coefficient is 0."""
    f = ell.es / (1.0 + math.sqrt(1.0 - ell.es))
    n = f / (2.0 - f)
    n2 = n * n
    n3, n4, n5, n6 = n2 * n, n2 * n2, n2 * n2 * n, n2 * n2 * n2
    cmu = [-3 / 2.0 * n + 9 / 16.0 * n3 - 3 / 32.0 * n5,
           15 / 16.0 * n2 - 15 / 32.0 * n4 + 135 / 2048.0 * n6,
           -35 / 48.0 * n3 + 105 / 256.0 * n5,
           315 / 512.0 * n4 - 189 / 512.0 * n6,
           -693 / 1280.0 * n5,
           1001 / 2048.0 * n6]
    cphi = [3 / 2.0 * n - 27 / 32.0 * n3 + 269 / 512.0 * n5,
            21 / 16.0 * n2 - 55 / 32.0 * n4 + 6759 / 4096.0 * n6,
            151 / 96.0 * n3 - 417 / 128.0 * n5,
            1097 / 512.0 * n4 - 15543 / 2560.0 * n6,
            8011 / 2560.0 * n5,
            293393 / 61440.0 * n6]
    return cmu, cphi


class Sinusoidal:
    """PROJ sinu, ellipsoidal (gn_sinu.cpp e_forward / e_inverse): x = lam cos phi /
    sqrt(1 - es sin^2 phi), y = the meridian arc M(phi).  The arc and its inverse
    are one 6-term Clenshaw sum each over the rectifying latitude (no
    ``pj_inv_mlfn`` iteration).  Outside the lobes (|y| beyond the pole's arc or
    |lam| > pi) both results are +inf; within 1e-10 of a pole lam = 0."""

    def __init__(self, ell: Ellipsoid):
        self.ell = ell
        self.Qn = TransverseMercator(ell, 1.0).Qn
        self.cmu, self.cphi = _rectifying_series(ell)

    def forward(self, lam, phi):
        lam = np.asarray(lam, dtype=np.float64)
        phi = np.asarray(phi, dtype=np.float64)
        s, c = np.sin(phi), np.cos(phi)
        x = lam * c / np.sqrt(1.0 - self.ell.es * s * s)
        y = self.Qn * _gatg(self.cmu, phi, (c - s) * (c + s), 2.0 * s * c)
        return x, y

    def inverse(self, x, y):
        x = np.asarray(x, dtype=np.float64)
        mu = np.asarray(y, dtype=np.float64) / self.Qn
        with np.errstate(invalid="ignore"):
            phi = _gatg(self.cphi, mu, np.cos(2 * mu), np.sin(2 * mu))
            s, c = np.sin(phi), np.cos(phi)
            away = np.abs(phi) - _HALFPI
            pole = np.abs(away) < _EPS10
            lam = np.where(pole, 0.0, x * np.sqrt(1.0 - self.ell.es * s * s) / c)
            bad = (away >= _EPS10) | (np.abs(lam) > math.pi + 1e-12)
        return np.where(bad, np.inf, lam), np.where(bad, np.inf, phi)


# ---- Rotated pole (PROJ ob_tran.cpp o_forward / o_inverse around longlat) ----------
def _aatan2(n, d):
    """PROJ aatan2: 0 where both arguments vanish."""
    return np.where((np.abs(n) < 1e-50) & (np.abs(d) < 1e-50), 0.0, np.arctan2(n, d))


class RotatedPole:
    """CF ``rotated_latitude_longitude``: PROJ ``+proj=ob_tran +o_proj=longlat
    +o_lat_p=pole_lat +o_lon_p=pole_grid_lon +lon_0=pole_lon + 180``.  A
    spherical rotation of (lon, lat); ``forward`` takes geographic degrees to
    rotated degrees, ``inverse`` the other way."""

    def __init__(self, pole_lat: float, pole_lon: float, pole_grid_lon: float = 0.0):
        from .crs import _DEG_TO_RAD
        self.lam0 = ((pole_lon + 360.0) % 360.0 - 180.0) * _DEG_TO_RAD   # lon_0, in [-180, 180)
        self.lamp = pole_grid_lon * _DEG_TO_RAD
        phip = pole_lat * _DEG_TO_RAD
        self.sphip, self.cphip = math.sin(phip), math.cos(phip)

    def forward(self, lon, lat):
        from .crs import _DEG_TO_RAD, _RAD_TO_DEG_FACTOR, _adjlon
        lam = _adjlon(np.asarray(lon, dtype=np.float64) * _DEG_TO_RAD - self.lam0)
        phi = np.asarray(lat, dtype=np.float64) * _DEG_TO_RAD
        sinlam, coslam = np.sin(lam), np.cos(lam)
        sinphi, cosphi = np.sin(phi), np.cos(phi)
        lam = _adjlon(_aatan2(cosphi * sinlam, self.sphip * cosphi * coslam + self.cphip * sinphi)
                      + self.lamp)
        phi = np.arcsin(np.clip(self.sphip * sinphi - self.cphip * cosphi * coslam, -1.0, 1.0))
        return lam * _RAD_TO_DEG_FACTOR, phi * _RAD_TO_DEG_FACTOR

    def inverse(self, rlon, rlat):
        from .crs import _DEG_TO_RAD, _RAD_TO_DEG_FACTOR, _adjlon
        lam = np.asarray(rlon, dtype=np.float64) * _DEG_TO_RAD - self.lamp
        phi = np.asarray(rlat, dtype=np.float64) * _DEG_TO_RAD
        sinlam, coslam = np.sin(lam), np.cos(lam)
        sinphi, cosphi = np.sin(phi), np.cos(phi)
        phi = np.arcsin(np.clip(self.sphip * sinphi + self.cphip * cosphi * coslam, -1.0, 1.0))
        lam = _aatan2(cosphi * sinlam, self.sphip * cosphi * coslam - self.cphip * sinphi)
        lam = _adjlon(lam + self.lam0)
        return lam * _RAD_TO_DEG_FACTOR, phi * _RAD_TO_DEG_FACTOR
