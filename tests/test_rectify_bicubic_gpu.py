"""Bicubic on the rectify route (K6q: xrs_rectify_var with XRS_INTERP_BICUBIC,
include/xrs.h) against a plain numpy float64 restatement with the kernel's
operation order, bit for bit."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from helpers import assert_bitwise_equal
from test_affine_bicubic_gpu import _cast

TILE_W, TILE_H = 32, 16   # K6q's target tile (xrs_rectify_bicubic.hip)
H, W = 23, 37             # the crafted case's source


def _weights(d):
    return [((-0.5 * d + 1.0) * d - 0.5) * d, (1.5 * d - 2.5) * (d * d) + 1.0,
            ((-1.5 * d + 2.0) * d + 0.5) * d, (0.5 * d - 0.5) * (d * d)]


def _classify(ij, h, w):   # (valid, i0, j0) of positions ij (2, H', W') over an h x w source
    fi, fj = ij
    with np.errstate(invalid="ignore"):
        ok = (fi >= 0) & (fi < w) & (fj >= 0) & (fj < h)
    return ok, np.where(ok, fi, 0).astype(np.int32), np.where(ok, fj, 0).astype(np.int32)


def bicubic_ref(data, ij, fill, cast=True):
    """(n, h, w) `data` at `ij`: the float64 sums (cast=False) or the output."""
    _, h, w = data.shape
    ok, i0, j0 = _classify(ij, h, w)
    wx, wy = _weights(np.where(ok, ij[0] - i0, 0.0)), _weights(np.where(ok, ij[1] - j0, 0.0))
    cols = [np.clip(i0 - 1 + b, 0, w - 1) for b in range(4)]
    val = data.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        hr = [((wx[0] * val[:, r, cols[0]] + wx[1] * val[:, r, cols[1]])
               + wx[2] * val[:, r, cols[2]]) + wx[3] * val[:, r, cols[3]]
              for r in (np.clip(j0 - 1 + a, 0, h - 1) for a in range(4))]
        res = ((wy[0] * hr[0] + wy[1] * hr[1]) + wy[2] * hr[2]) + wy[3] * hr[3]
    if not cast:
        return np.where(ok, res, 0.0)
    return np.where(ok, _cast(res, data.dtype), np.float64(fill).astype(data.dtype))


def _run(data, ij, fill, knob=None, **kw):
    import torch
    from xcube_resampling_amd import _native, kernels

    src = data if isinstance(data, torch.Tensor) else torch.from_numpy(data).cuda()
    with _native.testing_knob(*(knob or ("rectify_bicubic_direct", 0))):
        return kernels.rectify_var(torch.from_numpy(ij).cuda(), src, "bicubic", fill,
                                   **kw).cpu().numpy()


def test_reference_returns_the_source_at_integer_positions():
    data = np.random.default_rng(1).standard_normal((2, 9, 11))
    jj, ii = np.mgrid[0:9, 0:11].astype(np.float64)
    assert_bitwise_equal(bicubic_ref(data, np.stack([ii, jj]), np.nan), data)


@functools.lru_cache(maxsize=None)
def _crafted_ij():
    """45 x 70 positions over the 23 x 37 source: a rotated, scaled map that
    overshoots on all four sides, clipped onto the border pixels."""
    r, c = np.mgrid[0:45, 0:70].astype(np.float64)
    x, y = 0.62 * (c - 34.5), 0.62 * (r - 22.0)
    ca, sa = np.cos(0.44), np.sin(0.44)
    ij = np.stack([np.clip(18.0 + ca * x - sa * y, 0, W - 1),
                   np.clip(11.0 + sa * x + ca * y, 0, H - 1)])
    ij[:, 5:12, 20:30] = np.round(ij[:, 5:12, 20:30])   # u = v = 0
    ij[:, 14:34, 30:66] = np.nan                         # holds the whole tile (1, 1)
    ij[0, 0:5, 3:9] = np.nan                             # patches cutting other tiles
    ij[1, 40:43, 10:20] = np.nan
    ok, i0, j0 = _classify(ij, H, W)
    for edge in (i0 < 1, i0 > W - 3, j0 < 1, j0 > H - 3, (ij[0] == i0) & (ij[1] == j0),
                 ij[0] == 0, ij[0] == W - 1, ij[1] == H - 1):
        assert (edge & ok).any()
    assert not ok[np.isnan(ij).any(0)].any() and np.isnan(ij).any()
    assert np.isnan(ij[:, 16:32, 32:64]).all()
    # K6q's staged elements per tile ((imax - imin + 4) | 1) * (jmax - jmin + 4)
    areas = []
    for tr in range(0, 45, TILE_H):
        for tc in range(0, 70, TILE_W):
            t = (slice(tr, tr + TILE_H), slice(tc, tc + TILE_W))
            if ok[t].any():
                ti, tj = i0[t][ok[t]], j0[t][ok[t]]
                areas.append(int(((ti.max() - ti.min() + 4) | 1) * (tj.max() - tj.min() + 4)))
    assert min(areas) < (min(areas) + max(areas)) // 2 < max(areas)
    return ij, (min(areas) + max(areas)) // 2   # elements: between the smallest and largest tile


def _source(dtype, special=False):
    rng = np.random.default_rng(4)
    lo, hi = (0 if dtype == "uint8" else -120), (2 ** 40 if dtype == "int64" else 250)
    buf = (rng.standard_normal((2, H + 2, W + 3)) if np.dtype(dtype).kind == "f"
           else rng.integers(lo, hi, (2, H + 2, W + 3))).astype(dtype)
    if special:
        buf[0, 5, 9], buf[1, 12, 20], buf[1, 1, 2] = np.nan, np.inf, -np.inf
    return buf


# staging budget: default; every tile on the 16-tap path; 8 bytes: below any
# tile's 4 x 5 elements; "mid": between the smallest and the largest rectangle
PATHS = [None, ("rectify_bicubic_direct", 1), ("rectify_bicubic_lds", 8), "mid"]


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS, ids=["default", "direct", "lds8", "ldsmid"])
@pytest.mark.parametrize("dtype,special", [("float32", False), ("float64", False),
                                           ("uint8", False), ("int16", False),
                                           ("int64", False), ("float32", True)])
def test_crafted_positions(dtype, special, path):
    import torch

    ij, mid = _crafted_ij()
    buf = _source(dtype, special)
    data = buf[:, 1:H + 1, 2:W + 2]   # a view: slice stride (H + 2) (W + 3), row stride W + 3
    fill = np.nan if data.dtype.kind == "f" else 7
    if path == "mid":
        path = ("rectify_bicubic_lds", mid * data.itemsize)
    out = _run(torch.from_numpy(buf).cuda()[:, 1:H + 1, 2:W + 2], ij, fill, path)
    assert_bitwise_equal(out, bicubic_ref(data, ij, fill), f"{dtype} {path}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["uint8", "int16"])
def test_integer_overshoot_saturates(dtype):
    info = np.iinfo(dtype)
    jj, ii = np.mgrid[0:30, 0:30]
    data = np.where((ii // 3 + jj // 3) % 2, info.max, info.min).astype(dtype)[None]
    ij = np.random.default_rng(8).uniform(0, 29.99, (2, 40, 50))
    raw = bicubic_ref(data, ij, 0, cast=False)
    assert ((raw > info.max) | (raw < info.min)).sum() >= 20
    assert_bitwise_equal(_run(data, ij, 0), bicubic_ref(data, ij, 0))


@pytest.mark.gpu
def test_scattered_positions_take_the_global_path():
    # every tile's rectangle is the whole 300 x 300 float64 source (720 KB), beyond any LDS
    rng = np.random.default_rng(2)
    data = rng.standard_normal((1, 300, 300))
    ij = rng.uniform(0, 299.99, (2, 64, 64))
    assert_bitwise_equal(_run(data, ij, np.nan), bicubic_ref(data, ij, np.nan))


@pytest.mark.gpu
def test_through_the_layers():
    import torch
    import xcube_resampling_amd as xrs
    from test_rectify_gpu import _olci_like
    from xcube_resampling_amd import kernels, streaming
    from xcube_resampling_amd import rectify as R

    rng = np.random.default_rng(6)
    lon, lat = _olci_like(rng, 60, 50)
    a = rng.standard_normal((2, 60, 50)).astype(np.float32)
    b = rng.random((60, 50))
    coords = {"lon": (("y", "x"), lon), "lat": (("y", "x"), lat)}
    ds = xrs.Dataset(data_vars={"a": (("t", "y", "x"), a), "b": (("y", "x"), b)}, coords=coords)
    tgm = xrs.GridMapping.regular((120, 88), (4.99, 59.80), 0.0025, "EPSG:4326",
                                  tile_size=(32, 24))
    ij = R._compute_target_source_ij(xrs.GridMapping.from_dataset(ds), tgm, 1e-3)
    nij = ij.cpu().numpy()
    assert 0.2 < np.isnan(nij[0]).mean() < 0.8   # pixels outside the swath, and inside
    ref = bicubic_ref(a, nij, np.nan)
    bil = kernels.rectify_var(ij, torch.from_numpy(b[None]).cuda(), "bilinear", np.nan)
    methods = {"a": "bicubic", "b": "bilinear"}
    out = xrs.rectify_dataset(ds, target_gm=tgm, interp_methods=methods)
    assert_bitwise_equal(out["a"].values, ref, "a first, bicubic")
    assert_bitwise_equal(out["b"].values, bil.cpu().numpy()[0], "b: today's bilinear")
    only = xrs.Dataset(data_vars={"a": (("t", "y", "x"), a)}, coords=coords)
    for name, got in (
            ("only", xrs.rectify_dataset(only, target_gm=tgm, interp_methods="bicubic")),
            ("devices", xrs.rectify_dataset(ds, target_gm=tgm, interp_methods=methods,
                                            devices=[0, 0])),
            ("in_space", xrs.resample_in_space(only, target_gm=tgm, interp_methods="bicubic"))):
        assert_bitwise_equal(got["a"].values, ref, name)
    assert_bitwise_equal(streaming.rectify_host(a, ij, "bicubic", np.nan, band_rows=7,
                                                poison=True), ref, "rectify_host")
    assert_bitwise_equal(_run(a, nij, np.nan, rows=(5, 31)), ref[:, 5:31], "rows")
    with pytest.raises(NotImplementedError, match="interp_methods must be one of"):   # no fused K6q
        kernels.rectify_ij_var(None, None, None, tgm.height, tgm.width, tgm.x_res, -tgm.y_res,
                               1e-3, torch.from_numpy(a).cuda(), "bicubic", np.nan)
