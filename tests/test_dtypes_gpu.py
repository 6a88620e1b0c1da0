"""Every dispatched element type on every compute entry, against the oracles.

The other GPU modules run float32, float64, uint8 and int16 on small values.
Here int8, uint16, uint32, int32 and int64 run on the narrow range (0..200)
and on `wide` inputs: the full range of the type with planted extremes, so
that source-dtype differences wrap, scipy's output cast saturates, int64
values pass 2^53 and integer sums and products overflow.  Every comparison is
bit for bit (median by value, as test_coarsen_gpu does).  Every case names
the class of pixels it is there for and asserts, from the oracle, that at
least NEED pixels belong to it: a case that exercises nothing fails.

No input makes a NaN that is stored to an integer type: numpy's cast of NaN
is the host's (uint32 differs from the kernels' rule), and the reference never
reaches it (a NaN position raises IndexError first).
"""

from __future__ import annotations

import dataclasses
import functools
import math
import zlib

import numpy as np
import pytest

from helpers import assert_bitwise_equal
from oracle import affine_ref, gridmapping_ref as gref, rectify_ref, reproject_ref

pytestmark = pytest.mark.gpu

INT_DTYPES = ["int8", "uint16", "uint32", "int32", "int64"]
NEED = 20


def extremes(dtype) -> list[int]:
    """The values `wide` plants."""
    info = np.iinfo(dtype)
    vals = [info.min, info.min + 1, 0, 1, info.max - 1, info.max]
    if info.min < 0:
        vals.append(-1)
    if np.dtype(dtype) == np.int64:
        vals += [2**53 + 1, -(2**53 + 1), 2**62 + 3, -(2**62 + 3)]
    return vals


def wide(rng, dtype, shape):
    """Integers over the whole range of `dtype`: uniform draws (neighbours
    differ by more than half the range in one pair of four), one pixel in
    eight set to one of `extremes`, and 3 x 3 blocks of the minimum and of the
    maximum (one of each per 150 pixels of a slice) so that interpolated
    values reach both ends of the range too."""
    dt = np.dtype(dtype)
    info = np.iinfo(dt)
    a = rng.integers(info.min, info.max, shape, dtype=dt, endpoint=True)
    flat = a.reshape(-1)
    vals = extremes(dt)
    k = max(1, flat.size // (8 * len(vals)))
    flat[rng.choice(flat.size, k * len(vals), replace=False)] = np.tile(np.array(vals, dt), k)
    h, w = a.shape[-2:]
    if h >= 8 and w >= 8:
        for sl in a.reshape((-1, h, w)):
            for v in (info.min, info.max):
                for _ in range(max(2, h * w // 150)):
                    j, i = int(rng.integers(0, h - 2)), int(rng.integers(0, w - 2))
                    sl[j:j + 3, i:i + 3] = v
    return a


def narrow(rng, dtype, shape):
    return rng.integers(0, min(200, np.iinfo(dtype).max), shape).astype(dtype)


def make(kind, rng, dtype, shape):
    return (wide if kind == "wide" else narrow)(rng, dtype, shape)


def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def need(count, what):
    assert int(count) >= NEED, f"only {int(count)} pixels of the class under test: {what}"


def outside(ref, dtype):
    """Pixels of a float64 result outside the range of `dtype`."""
    info = np.iinfo(dtype)
    return (ref > float(info.max)) | (ref < float(info.min))


def large(ref, dtype):
    """Pixels beyond a quarter of the positive range of `dtype` in magnitude
    (no narrow input reaches it)."""
    return np.abs(np.asarray(ref).astype(np.float64)) > float(np.iinfo(dtype).max // 4)


def beyond_narrow(ref, dtype):
    """Results no narrow input of a selecting or averaging reducer makes."""
    return (ref < 0) | (ref >= min(200, np.iinfo(dtype).max))


def folds_wrap(agg, dtype, npix):
    """True where sums / products of `npix` full-range values of `dtype` leave
    the 64-bit result type (then the wide case must show wrapped results);
    else they must at least leave the source type."""
    bits = 8 * np.dtype(dtype).itemsize
    return (agg == "sum" and bits == 64) or (agg == "prod" and bits * npix > 80)


def count_fold(ref, exact, agg, dtype, npix):
    """Windows whose exact sum / product overflows 64 bits where `folds_wrap`,
    else results beyond the source type."""
    if folds_wrap(agg, dtype, npix):
        return int((exact() != ref.astype(object)).sum())
    return int((np.abs(ref.astype(np.float64)) > float(np.iinfo(dtype).max)).sum())


def count_reduced(ref, exact, agg, dtype, kind, npix):
    """Pixels of a reducer's result in the class its case is there for."""
    if kind == "narrow" or agg == "count":
        return int((ref != 0).sum())
    if agg in ("sum", "prod"):
        return count_fold(ref, exact, agg, dtype, npix)
    return int(beyond_narrow(ref, dtype).sum())


def at_limits(ref, dtype):
    info = np.iinfo(dtype)
    return (ref == info.min) | (ref == info.max)


def _host(t):
    return t if isinstance(t, np.ndarray) else t.cpu().numpy()


# ------------------------------------------------------------------ K1 -------
# 96 x 80 EPSG:4326 source -> 150 x 70 EPSG:3857 target in 64 x 48 tiles (3 x 2,
# partial tiles on both axes); the target reaches 2 to 10 pixels beyond the
# source on all four sides (fill)
K1_W, K1_H, K1_XR, K1_YR = 96, 80, 0.0075, 0.005
K1_TARGET = ((150, 70), (-560000.0, 7280000.0), (600.0, 1200.0), (64, 48))
K1_FILL = 7


@functools.lru_cache(maxsize=None)
def k1_geometry():
    lon = -5.0 + (np.arange(K1_W) + 0.5) * K1_XR
    lat = 55.0 - (np.arange(K1_H) + 0.5) * K1_YR
    tsize, tmin, tres, ttile = K1_TARGET
    return lon, lat, gref.regular_geometry(tsize, tmin, tres, tile_size=ttile)


def _k1_bounds(*b):
    return gref.transform_bounds(gref.webmerc_inverse, *b)


def k1_oracle(data, interp):
    lon, lat, geo = k1_geometry()
    ttile = K1_TARGET[3]
    return reproject_ref.reproject_array(
        data, gref.webmerc_inverse, _k1_bounds, lon, lat, K1_XR, K1_YR, geo["x_coords"],
        geo["y_coords"], geo["xy_bboxes"], ttile[0], ttile[1], interp, K1_FILL)


def k1_triangular_prestore(data):
    """The float64 values reproject_block's triangular branch computes
    (reproject.py:316-335), before their assignment into the source-dtype
    output casts them."""
    lon, lat, geo = k1_geometry()
    (dw, dh), _, _, (tw, th) = K1_TARGET
    ntx, nty = math.ceil(dw / tw), math.ceil(dh / th)
    b, xc, yc, pad = reproject_ref.get_scr_bboxes_indices(
        _k1_bounds, lon, lat, K1_XR, K1_YR, K1_W, K1_H, geo["xy_bboxes"], ntx, nty)
    out = np.zeros((data.shape[0], dh, dw), np.float64)
    for j in range(nty):
        for i in range(ntx):
            sl = np.s_[j * th:(j + 1) * th, i * tw:(i + 1) * tw]
            xx, yy = np.meshgrid(geo["x_coords"][sl[1]], geo["y_coords"][sl[0]])
            sxx, syy = gref.webmerc_inverse(xx, yy)
            win = reproject_ref._padded_window(data, pad, b[:, j, i], K1_FILL)
            ix = (sxx - xc[:1, j, i]) / K1_XR
            iy = (syy - yc[:1, j, i]) / -K1_YR
            fx, cx = np.floor(ix).astype(np.int16), np.ceil(ix).astype(np.int16)
            fy, cy = np.floor(iy).astype(np.int16), np.ceil(iy).astype(np.int16)
            dx, dy = ix - fx, iy - fy
            v00, v01, v10, v11 = win[:, fy, fx], win[:, fy, cx], win[:, cy, fx], win[:, cy, cx]
            lower = v00 + dx * (v01 - v00) + dy * (v10 - v00)
            upper = v11 + (1.0 - dx) * (v10 - v11) + (1.0 - dy) * (v01 - v11)
            out[(slice(None),) + sl] = np.where(dx + dy < 1.0, lower, upper)
    return out


@functools.lru_cache(maxsize=None)
def _k1_plans():
    import xcube_resampling_amd as xrs

    lon, lat, geo = k1_geometry()
    tsize, tmin, tres, ttile = K1_TARGET
    ds = xrs.Dataset(data_vars={"v": (("t", "lat", "lon"), np.zeros((1, K1_H, K1_W), np.uint8))},
                     coords={"lon": ("lon", lon), "lat": ("lat", lat)})
    sgm = xrs.GridMapping.from_dataset(ds)
    tgm = xrs.GridMapping.regular(tsize, tmin, tres, "EPSG:3857", tile_size=ttile)
    plan = xrs.plan_reproject(sgm, tgm, xrs.Transformer.from_crs(tgm.crs, sgm.crs,
                                                                  always_xy=True))
    assert plan.coord_mode == 0 and plan.x_gen is not None
    table = dataclasses.replace(plan, x_gen=None, _device_cache={})
    xx, yy = np.meshgrid(geo["x_coords"], geo["y_coords"])
    sx, sy = gref.webmerc_inverse(xx, yy)
    table2d = dataclasses.replace(plan, coord_mode=1, src_x=sx, src_y=sy, x_gen=None,
                                  _device_cache={})
    return {"gen": plan, "table": table, "2d": table2d}


@pytest.mark.parametrize("kind", ["narrow", "wide"])
@pytest.mark.parametrize("dtype", INT_DTYPES)
def test_reproject_all_dtypes(dtype, kind):
    """K1 nearest, bilinear (float64; float32 too for int32) and triangular
    with generated columns (coord_mode 2) and the src_x table (coord_mode 0),
    int32 and int64 also with 2-D tables (coord_mode 1).  Classes — narrow:
    pixels off the fill; wide nearest: values beyond a quarter of the range;
    wide bilinear: results outside the type's range (only a wrapped
    `v01 - v00` makes one); wide triangular: float64 values outside the type's
    range stored into it.

    uint32 runs no wide triangular case: numpy's float64 -> uint32 cast of a
    value of 2^32 or more is not one function of the value (test_dtypes_cpu.
    UINT32_ABOVE_RANGE), uint32 differences never wrap below zero, so every
    out-of-range store of that case is of this kind and the reference has no
    single answer for it; the narrow uint32 case asserts that it makes none."""
    import torch

    from xcube_resampling_amd import kernels

    dt = np.dtype(dtype)
    data = make(kind, _rng("k1", dtype, kind), dt, (2, K1_H, K1_W))
    src = torch.from_numpy(data).cuda()
    plans = _k1_plans()
    modes = ["gen", "table"] + (["2d"] if dtype in ("int32", "int64") else [])
    interps = ["nearest", "bilinear", "triangular"]
    if dtype == "uint32":
        if kind == "wide":
            interps.remove("triangular")
        else:
            assert not outside(k1_triangular_prestore(data), dt).any()
    for interp in interps:
        ref = k1_oracle(data, interp)
        assert ref.dtype == (np.float64 if interp == "bilinear" else dt)
        if kind == "narrow":
            need((ref != K1_FILL).sum(), f"{interp}: pixels off the fill")
        elif interp == "nearest":
            need(large(ref, dt).sum(), "nearest: values beyond a quarter of the range")
        elif interp == "bilinear":
            need(outside(ref, dt).sum(), "bilinear: wrapped source-dtype differences")
        else:
            pre = k1_triangular_prestore(data)
            assert_bitwise_equal(pre.astype(dt), ref, "triangular restatement")
            need(outside(pre, dt).sum(), "triangular: stores outside the type's range")
        for mode in modes:
            out = kernels.reproject(src, plans[mode], interp, K1_FILL)
            assert_bitwise_equal(out.cpu().numpy(), ref, f"{dtype} {kind} {interp} {mode}")
        if interp == "bilinear" and dtype == "int32":
            out = kernels.reproject(src, plans["gen"], interp, K1_FILL, out_dtype=np.float32)
            assert_bitwise_equal(out.cpu().numpy(), ref.astype(np.float32), "float32 out")


@pytest.mark.parametrize("dtype", ["uint32", "int32", "int64"])
def test_reproject_bicubic_wide(dtype):
    """K1q on the Mercator geometry of test_bicubic_gpu; class: results beyond
    a quarter of the range (int64: beyond 2^53, where int64 -> float64 rounds)."""
    from test_bicubic_gpu import MERC, _case, _run, bicubic_ref

    sgm, tgm, tr, plan, sx, sy, data = _case(*MERC, dtype, 1)
    data = wide(_rng("k1q", dtype), dtype, data.shape)
    ref = bicubic_ref(data, sgm, tgm, tr.transform_bounds, sx, sy, float(K1_FILL))
    need(large(ref, dtype).sum(), "bicubic: taps beyond a quarter of the range")
    if dtype == "int64":
        need((np.abs(ref) > 2.0**53).sum(), "bicubic: int64 taps beyond 2^53")
    assert_bitwise_equal(_run(plan, data, float(K1_FILL)), ref, dtype)


# ------------------------------------------------------------- K2 / K3 -------
def _affine(a, m, oshape, ochunks, order, agg, fill):
    import xcube_resampling_amd.affine as A

    ref = np.asarray(affine_ref.resample_array(a, m, oshape, ochunks, order, agg, False, fill))
    got = _host(A._resample_array(a, None, None, m, oshape, ochunks, order, agg, False, fill))
    return got, ref


@pytest.mark.parametrize("kind", ["narrow", "wide"])
@pytest.mark.parametrize("dtype", INT_DTYPES)
def test_affine_plain_all_dtypes(dtype, kind):
    """The plain branch (scipy order 0 and 1, no reducer) at scales 0.5, 1.0
    and 0.9216 with a fractional offset, 36 x 66 outputs in 16 x 24 chunks.
    Classes — narrow: pixels off the fill; wide: pixels that come out at a
    limit of the type (scipy's clamp at both ends; for int64 the upper end is
    INT64_MIN, and order 0 passes every value through float64)."""
    dt = np.dtype(dtype)
    a = make(kind, _rng("k2", dtype, kind), dt, (44, 72))
    for order in (0, 1):
        for scale in (0.5, 1.0, 0.9216):
            m = ((scale, 0.0, 1.3), (0.0, scale, 0.6))
            got, ref = _affine(a, m, (36, 66), (16, 24), order, "first", 7)
            what = f"{dtype} {kind} order={order} scale={scale}"
            if kind == "narrow":
                need((ref != 7).sum(), "pixels off the fill")
            else:
                need(at_limits(ref, dt).sum(), f"{what}: pixels at the limits of the type")
            assert_bitwise_equal(got, ref, what)
    if kind == "wide" and dtype == "int64":
        m = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0))
        for order in (0, 1):   # identity is not a copy for int64
            got, ref = _affine(a, m, (44, 72), (16, 24), order, "first", 7)
            need((ref != a).sum(), "identity: int64 values that float64 does not hold")
            need(((a > 2**62) & (ref == np.iinfo(dt).min)).sum(), "identity: top of the range")
            assert_bitwise_equal(got, ref, f"int64 identity order={order}")


def _exact_window_fold(up, dy, dx, agg):
    """Window sums / products of the div-x intermediate in Python integers."""
    h, w = up.shape[-2] // dy, up.shape[-1] // dx
    win = up.astype(object).reshape(up.shape[:-2] + (h, dy, w, dx))
    nd = win.ndim
    return win.sum(axis=(nd - 3, nd - 1)) if agg == "sum" else win.prod(axis=(nd - 3, nd - 1))


@pytest.mark.parametrize("kind", ["narrow", "wide"])
@pytest.mark.parametrize("dtype", INT_DTYPES)
@pytest.mark.parametrize("agg", ["mean", "sum", "prod", "max", "min", "count", "first", "center"])
def test_affine_coarsen_all_dtypes(agg, dtype, kind):
    """The fused coarsen at factor 4 on aligned grids and at factor 2.5.
    Classes (`count_reduced`) — narrow and count: non-zero results; wide
    sum and prod: windows whose exact sum / product does not fit the 64-bit
    result type (the result is the wrapped one) wherever `folds_wrap`, else
    results beyond the source type's range; the others: results no narrow
    input makes."""
    dt = np.dtype(dtype)
    rng = _rng("k3", agg, dtype, kind)
    for scale, off, oshape, tile in [(4.0, (0.0, 0.0), (20, 30), (8, 12)),
                                     (2.5, (1.1, 0.4), (24, 34), (24, 17))]:
        a = make(kind, rng, dt, (int(oshape[0] * scale) + 5, int(oshape[1] * scale) + 3))
        if kind == "narrow" and agg == "prod":
            a = rng.integers(1, 4, a.shape).astype(dt)
        m = ((scale, 0.0, off[0]), (0.0, scale, off[1]))
        got, ref = _affine(a, m, oshape, tile, 1, agg, 3)
        d = math.ceil(scale)

        def exact():
            up = affine_ref.upscale(a, ((scale / d, 0.0, off[0]), (0.0, scale / d, off[1])),
                                    (oshape[0] * d, oshape[1] * d), tile, 1, False, 3)
            return _exact_window_fold(np.asarray(up), d, d, agg)

        need(count_reduced(ref, exact, agg, dt, kind, d * d), f"{agg} {dtype} {kind} {scale}")
        assert_bitwise_equal(got, ref, f"{agg} {dtype} {kind} scale={scale}")


@pytest.mark.parametrize("dtype", INT_DTYPES)
def test_affine_bicubic_wide(dtype):
    """K2q, product path and the direct kernel; class: pixels the cubic's
    overshoot saturates at a limit of the type (int64's upper limit comes out
    as INT64_MIN, see _cast)."""
    from test_affine_bicubic_gpu import GEOMETRIES, _plan, _run, bicubic_ref

    scale, offset, shape = GEOMETRIES[0]
    data = wide(_rng("k2q", dtype), dtype, (1,) + shape)
    plan = _plan(data.shape, dtype, scale, offset, (150, 200), (64, 48), 7.0)
    ref = bicubic_ref(data, plan)
    need(at_limits(ref, np.dtype(dtype)).sum(), "bicubic: saturated pixels")
    assert_bitwise_equal(_run(plan, data), ref, f"K2q {dtype}")
    assert_bitwise_equal(_run(plan, data, ("affine_bicubic_direct", 1)), ref, f"direct {dtype}")


# ------------------------------------------------------------------ K7 -------
K7_WINDOWS = [(2, 2), (3, 9), (8, 8)]
K7_WIDE_AGGS = ["mean", "sum", "prod", "max", "min", "median", "std", "var", "first", "last",
                "center", "count"]   # mode's histogram is indexed by value: narrow only


def _k7(agg, dtype, kind):
    from test_coarsen_gpu import _check, _coarsen_gpu

    dt = np.dtype(dtype)
    rng = _rng("k7", agg, dtype, kind)
    cases = []
    for dy, dx in K7_WINDOWS:
        shape = (2, dy * int(rng.integers(10, 16)), dx * int(rng.integers(10, 16)))
        a = make(kind, rng, dt, shape)
        if kind == "narrow" and agg == "prod":
            a = rng.integers(1, 4, shape).astype(dt)
        chunks = (1, dy * 2 + 1, dx * 3)   # unaligned chunks: dask rechunks them
        ref = np.asarray(affine_ref.coarsen_chunked(agg, a, {1: dy, 2: dx}, chunks))
        cases.append((a, dy, dx, chunks, ref, count_reduced(
            ref, lambda: _exact_window_fold(a, dy, dx, agg), agg, dt, kind, dy * dx)))
    # (windows of 64 full-range values nearly always hold a zero or overflow to
    # zero: the class is counted over the three windows of the case)
    need(sum(c[-1] for c in cases), f"{agg} {dtype} {kind}")
    for a, dy, dx, chunks, ref, _ in cases:
        _check(_coarsen_gpu(a, dy, dx, agg, chunks), ref, agg, f"{agg} {dtype} {kind} {dy}x{dx}")


@pytest.mark.parametrize("dtype", ["int8", "uint16", "uint32", "int32"])
@pytest.mark.parametrize("agg", ["mean", "sum", "max", "min", "prod", "count", "first", "last",
                                 "center", "median", "mode", "std", "var"])
def test_coarsen_narrow_all_dtypes(agg, dtype):
    _k7(agg, dtype, "narrow")


# (var of full-range uint32 windows is ~1e18: numpy's cast of it to uint32 is
# the host-specific one described at test_reproject_all_dtypes)
@pytest.mark.parametrize("agg,dtype", [(a, d) for a in K7_WIDE_AGGS
                                       for d in ("uint32", "int32", "int64")
                                       if (a, d) != ("var", "uint32")])
def test_coarsen_wide(agg, dtype):
    _k7(agg, dtype, "wide")


# ------------------------------------------------------------- K6 / K5 -------
K6_SRC = (50, 64)    # source rows, columns
K6_DST = (60, 70)


@functools.lru_cache(maxsize=None)
def k6_positions():
    """A 60 x 70 image of source positions (i, j) over the 50 x 64 source:
    uniform fractions, then rows and columns of integral positions, of
    positions on the last column / row, of fractions exactly 0.5 (nearest
    takes the upper neighbour only for u > 0.5) and a NaN block."""
    rng = _rng("k6 positions")
    (sh, sw), (dh, dw) = K6_SRC, K6_DST
    ij = np.stack([rng.uniform(0, sw - 1, (dh, dw)), rng.uniform(0, sh - 1, (dh, dw))])
    ij[:, 5:9] = np.floor(ij[:, 5:9])
    ij[0, 12:15] = sw - 1
    ij[1, :, 20:23] = sh - 1
    ij[:, 30:34] = np.floor(ij[:, 30:34] * 0.98) + 0.5
    ij[0, 40:43] = np.floor(ij[0, 40:43])
    ij[0, 40:43, ::2] += 0.5
    ij[:, 48:55, 33:47] = np.nan
    assert np.nanmax(ij[0]) <= sw - 1 and np.nanmax(ij[1]) <= sh - 1 and np.nanmin(ij) >= 0
    return ij


def _k6_var(dtype, key):
    rng = _rng("k6", dtype, key)
    if dtype == "float64":
        return rng.standard_normal((2,) + K6_SRC), float("nan")
    return wide(rng, dtype, (2,) + K6_SRC), 7


def _k6_need(ref, dtype, fill, what):
    if dtype == "float64":
        need(np.isfinite(ref).sum(), f"{what}: sampled pixels")
    else:
        need(large(ref, dtype).sum(), f"{what}: samples beyond a quarter of the range")
        if dtype == "int64":
            need((np.abs(ref.astype(np.float64)) > 2.0**53).sum(), f"{what}: beyond 2^53")


@pytest.mark.parametrize("dtype", INT_DTYPES + ["float64"])
def test_rectify_var_all_dtypes(dtype):
    """K6 at synthetic positions, all three interpolations."""
    import torch

    from xcube_resampling_amd import kernels

    ij = k6_positions()
    var, fill = _k6_var(dtype, "unfused")
    dev_ij, src = torch.from_numpy(ij).cuda(), torch.from_numpy(var).cuda()
    for interp in ("nearest", "bilinear", "triangular"):
        ref = rectify_ref.compute_var_image(ij, var, fill, interp, (32, 24))
        _k6_need(ref, dtype, fill, f"{dtype} {interp}")
        out = kernels.rectify_var(dev_ij, src, interp, fill)
        assert_bitwise_equal(out.cpu().numpy(), ref, f"{dtype} {interp}")


def fused_swath():
    """(source grid mapping, target grid mapping, device (lon, lat), source
    (h, w)) of test_fused_resolve_sampling_equals_k5_then_k6: a jittered swath
    with NaN coordinates and a degenerate quad, 40 x 36 target tiles."""
    import torch

    import xcube_resampling_amd as xrs

    rng = np.random.default_rng(17)
    h, w = 110, 95
    jj, ii = np.mgrid[0:h, 0:w].astype(np.float64)
    lon = 3.0 + 0.01 * ii + 0.002 * jj + rng.normal(0, 0.002, (h, w))
    lat = 40.0 - 0.008 * jj + 0.001 * ii + rng.normal(0, 0.002, (h, w))
    lat[40:42, 20] = np.nan
    lon[60, 5] = lon[60, 4]
    sgm = xrs.GridMapping.from_coords(xrs.DataArray(lon, ("y", "x"), name="lon"),
                                      xrs.DataArray(lat, ("y", "x"), name="lat"), "EPSG:4326")
    res = 0.006
    x0 = float(np.floor(np.nanmin(lon) / res) * res)
    y0 = float(np.floor(np.nanmin(lat) / res) * res)
    size = (int(np.ceil((np.nanmax(lon) - x0) / res)), int(np.ceil((np.nanmax(lat) - y0) / res)))
    tgm = xrs.GridMapping.regular(size, (x0, y0), res, "EPSG:4326", tile_size=(40, 36))
    return sgm, tgm, (torch.from_numpy(lon).cuda(), torch.from_numpy(lat).cuda()), (h, w)


@pytest.mark.parametrize("dtype", INT_DTYPES + ["float64"])
def test_rectify_fused_all_dtypes(dtype):
    """xrs_rectify_ij_var == K5 then K6 on the swath of
    test_fused_resolve_sampling_equals_k5_then_k6, and both == the oracle's
    samples at K5's positions."""
    import torch

    from xcube_resampling_amd import kernels
    from xcube_resampling_amd import rectify as R

    sgm, tgm, xy, (h, w) = fused_swath()
    rng = _rng("k5k6", dtype)
    if dtype == "float64":
        var, fill = rng.standard_normal((2, h, w)), float("nan")
    else:
        var, fill = wide(rng, dtype, (2, h, w)), 7
    src = torch.from_numpy(var).cuda()
    tiles = R._device_tiles(sgm, tgm, xy)
    ij = kernels.rectify_ij(xy[0], xy[1], tiles, 0, tgm.height, tgm.width, tgm.x_res,
                            -tgm.y_res, 1e-3)
    ij_host = ij.cpu().numpy()
    for interp in ("nearest", "bilinear", "triangular"):
        ref = rectify_ref.compute_var_image(ij_host, var, fill, interp, (40, 36))
        _k6_need(ref, dtype, fill, f"fused {dtype} {interp}")
        exp = kernels.rectify_var(ij, src, interp, fill).cpu().numpy()
        assert_bitwise_equal(exp, ref, f"K6 {dtype} {interp}")
        _, got = kernels.rectify_ij_var(xy[0], xy[1], R._device_tiles(sgm, tgm, xy), tgm.height,
                                        tgm.width, tgm.x_res, -tgm.y_res, 1e-3, src, interp,
                                        fill, keep_ij=False)
        assert_bitwise_equal(got.cpu().numpy(), exp, f"fused {dtype} {interp}")
