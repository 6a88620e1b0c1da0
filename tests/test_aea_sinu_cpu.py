"""Albers and sinusoidal restatements against mpmath (50 digits: Snyder's
(14-1)..(14-11) with the latitude by findroot on the q equation, and the meridian
arc by mp.ellipe with findroot back), analytic points, CF round trips.
Worst |numpy - mpmath| on these 33 x 33 grids (pole to pole, lon_0 - 180 .. lon_0 +
180; the inverses take the forward results, so they reach the domain edges):
Albers forward 8.9e-9 m, inverse 3.93e-13 deg; sinusoidal forward 5.5e-9 m, inverse
1.28e-13 deg.  BOUND is 4 x those (rounding spread across libm builds), below the
device-versus-numpy bar of tests/test_transform_gpu.py (1e-7 m, 1e-12 deg), with one
exception: 4 x the Albers inverse's 3.93e-13 deg would be 1.6e-12, so that bound is the
bar itself (a margin of 2.5).  Its worst rows are the two 5.6 deg from a pole
(3.5e-13 .. 3.9e-13 deg; 1.9e-13 at most on every other row): q is flat there, dphi =
dq / (2 cos phi), and the one rounding of PROJ's frame, (x - x0) * ra, is already 1.2e-15
of q at the far pole's radius, 3.5e-13 deg.
The pole rows follow PROJ's rules in both columns: Albers takes |q| within 1e-7 of
qp as the pole (no other grid row lies in that band, 0.026 deg wide), and the
sinusoidal longitude within 1e-10 rad of a pole is lon_0."""
import mpmath as mp
import numpy as np
import pytest

from xcube_resampling_amd.crs import CRS, Transformer, sinusoidal_crs

mp.mp.dps = 50
RAD = mp.pi / 180
BOUND = {"aea": (3.6e-8, 1.0e-12), "sinu": (2.3e-8, 5.2e-13)}   # (forward m, inverse deg)
RF = {"WGS 84": "298.257223563", "GRS 1980": "298.257222101"}


def _cf_aea(sp, lat_0, lon_0, fe=0.0, fn=0.0):
    return CRS.from_cf(dict(grid_mapping_name="albers_conical_equal_area", standard_parallel=sp,
                            latitude_of_projection_origin=lat_0,
                            longitude_of_central_meridian=lon_0, false_easting=fe,
                            false_northing=fn))


CASES = {
    "EPSG:5070": lambda: CRS.from_epsg(5070),
    "EPSG:3577": lambda: CRS.from_epsg(3577),                       # n < 0
    "1SP": lambda: _cf_aea(40.0, 40.0, 10.0, 1.0e6, 2.0e6),         # WGS 84
    "MODIS": lambda: sinusoidal_crs(),
    "sinu WGS 84": lambda: sinusoidal_crs(20.0, 6378137.0, 298.257223563, 5.0e5, 1.0e6),
}


def _tr(a, b):
    return Transformer.from_crs(a, b, always_xy=True)


def _mp_aea(crs):
    """(forward, inverse) in mpmath, Snyder (14-1)..(14-11), degrees <-> metres."""
    f = 1 / mp.mpf(RF[crs.params[0]])
    a, e = mp.mpf(6378137), mp.sqrt(2 * f - f * f)
    lon_0, lat_0, _, fe, fn, lat_1, lat_2 = crs.params[1:8]

    def m(p):
        return mp.cos(p) / mp.sqrt(1 - (e * mp.sin(p)) ** 2)

    def q(p):
        s = e * mp.sin(p)
        return (1 - e * e) * (mp.sin(p) / (1 - s * s) - mp.log((1 - s) / (1 + s)) / (2 * e))

    p1, p2, qp = lat_1 * RAD, lat_2 * RAD, q(mp.pi / 2)
    n = mp.sin(p1) if lat_1 == lat_2 else (m(p1) ** 2 - m(p2) ** 2) / (q(p2) - q(p1))
    big_c = m(p1) ** 2 + n * q(p1)
    rho0 = a * mp.sqrt(big_c - n * q(lat_0 * RAD)) / n

    def fwd(lon, lat):
        rho, th = a * mp.sqrt(big_c - n * q(mp.mpf(lat) * RAD)) / n, n * (mp.mpf(lon) - lon_0) * RAD
        return fe + rho * mp.sin(th), fn + rho0 - rho * mp.cos(th)

    def inv(x, y, guess):
        dx, dy, sgn = mp.mpf(x) - fe, rho0 - (mp.mpf(y) - fn), mp.sign(n)
        qq = (big_c - (dx * dx + dy * dy) * n * n / (a * a)) / n
        if abs(qp - abs(qq)) <= mp.mpf("1e-7"):
            phi = mp.sign(qq) * mp.pi / 2
        else:
            phi = mp.findroot(lambda p: q(p) - qq, mp.mpf(guess) * RAD)
        return lon_0 + mp.atan2(sgn * dx, sgn * dy) / n / RAD, phi / RAD

    return fwd, inv


def _mp_sinu(crs):
    """(forward, inverse) in mpmath: the meridian arc a (E(phi | es) - es sin cos / sqrt(1 -
    es sin^2)) by mp.ellipe."""
    lon_0, _, _, fe, fn, a, rf = crs.params[1:8]
    a, f = mp.mpf(a), (1 / mp.mpf(RF.get(crs.params[0], rf)) if rf else mp.mpf(0))
    es = 2 * f - f * f

    def arc(p):
        return mp.ellipe(p, es) - es * mp.sin(p) * mp.cos(p) / mp.sqrt(1 - es * mp.sin(p) ** 2)

    def fwd(lon, lat):
        lam, phi = (mp.mpf(lon) - lon_0) * RAD, mp.mpf(lat) * RAD
        return (fe + a * lam * mp.cos(phi) / mp.sqrt(1 - es * mp.sin(phi) ** 2), fn + a * arc(phi))

    def inv(x, y, guess):
        phi = mp.findroot(lambda p: arc(p) - (mp.mpf(y) - fn) / a, mp.mpf(guess) * RAD)
        if abs(abs(phi) - mp.pi / 2) < mp.mpf("1e-10"):
            return mp.mpf(lon_0), phi / RAD
        lam = (mp.mpf(x) - fe) * mp.sqrt(1 - es * mp.sin(phi) ** 2) / (a * mp.cos(phi))
        return lon_0 + lam / RAD, phi / RAD

    return fwd, inv


def _err(got, fn, *args, wrap=True):
    """max |numpy - mpmath| over both coordinates (longitudes modulo 360)."""
    exp = [fn(*a) for a in zip(*(v.ravel() for v in args))]
    dx = [abs((g - e[0] + 180) % 360 - 180) if wrap else abs(g - e[0]) for g, e in zip(got[0].ravel(), exp)]
    return float(max(dx + [abs(g - e[1]) for g, e in zip(got[1].ravel(), exp)]))


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_against_mpmath(name):
    crs = CASES[name]()
    fwd, inv = (_mp_aea if crs.kind == "aea" else _mp_sinu)(crs)
    lon, lat = np.meshgrid(crs.params[1] + np.linspace(-180, 180, 33), np.linspace(-90, 90, 33))
    xy = _tr("EPSG:4326", crs).transform(lon, lat)
    err = _err(xy, fwd, lon, lat, wrap=False)
    geo = _tr(crs, "EPSG:4326").transform(*xy)
    assert np.isfinite(geo).all()
    ierr = _err(geo, inv, *xy, lat)
    print(f"{name}: forward {err:.3g} m, inverse {ierr:.3g} deg")
    assert err <= BOUND[crs.kind][0] < 1e-7 and ierr <= BOUND[crs.kind][1] <= 1e-12


@pytest.mark.parametrize("name", list(CASES))
def test_analytic_points(name):
    crs = CASES[name]()
    tr, back, (lon_0, lat_0, _, fe, fn) = _tr("EPSG:4326", crs), _tr(crs, "EPSG:4326"), crs.params[1:6]
    np.testing.assert_allclose(tr.transform(lon_0, lat_0), (fe, fn), rtol=0, atol=1e-9)
    lat = np.array([-90.0, -37.0, 0.0, 52.0, 90.0])
    mx, my = tr.transform(np.full(5, lon_0), lat)                    # the central meridian
    assert (mx == fe).all() and (np.diff(my) > 0).all()
    blon, blat = back.transform(mx, my)
    np.testing.assert_allclose(blon, lon_0, rtol=0, atol=1e-13)     # lam = 0; lam0's round trip
    np.testing.assert_allclose(blat, lat, rtol=0, atol=1e-12)
    inf2 = (np.inf, np.inf)
    if crs.kind == "aea":   # the pole select; 10 km beyond either pole's arc: outside
        assert (blat[[0, 4]] == (-90.0, 90.0)).all()
        assert back.transform(fe, my[4] + 1.0e4) == inf2 and back.transform(fe, my[0] - 1.0e4) == inf2
        return
    a = crs.params[6]
    assert back.transform(fe, my[4] + 1.0) == inf2 and back.transform(fe, my[0] - 1.0) == inf2
    assert back.transform(fe + 0.75 * np.pi * a, fn + 0.25 * np.pi * a) == inf2   # between the lobes
    assert np.isfinite(back.transform(fe + 0.70 * np.pi * a, fn + 0.25 * np.pi * a)).all()
    if name == "MODIS":     # the sphere's closed form: the series adds zeros and one rounding
        lon, lat = np.meshgrid(np.linspace(-180, 180, 25), np.linspace(-90, 90, 19))
        x, y = tr.transform(lon, lat)
        np.testing.assert_allclose(x, a * np.radians(lon) * np.cos(np.radians(lat)), rtol=1e-15, atol=1e-9)
        np.testing.assert_allclose(y, a * np.radians(lat), rtol=1e-15)


@pytest.mark.parametrize("name", list(CASES))
def test_cf_round_trip(name):
    crs = CASES[name]()
    cf = crs.to_cf()
    assert CRS.from_cf(cf).equals(crs) and crs.is_projected
    assert not _tr("EPSG:4326", crs).is_separable
    if crs.authority == "EPSG":   # the parameters alone: the registry entry
        assert CRS.from_cf({k: v for k, v in cf.items() if k != "crs_wkt"}) is crs
        assert CRS.from_string(crs.code) is crs
    if crs.kind == "sinu":
        cf["longitude_of_central_meridian"] = cf.pop("longitude_of_projection_origin")
        assert CRS.from_cf(cf).equals(crs)


def test_sinusoidal_figures_and_codes():
    assert sinusoidal_crs().params[6:8] == (6371007.181, 0.0)
    by_b = CRS.from_cf(dict(grid_mapping_name="sinusoidal", semi_major_axis=6378137.0,
                            semi_minor_axis=6356752.314245179))
    assert abs(by_b.params[7] - 298.257223563) < 1e-6
    assert [CRS.from_epsg(c).params[6:8] for c in (5070, 3577, 3005)] == \
        [(29.5, 45.5), (-18.0, -36.0), (50.0, 58.5)]
    assert CRS.from_epsg(3005).params[4:6] == (1000000.0, 0.0)
