"""Bicubic reprojection (XRS_INTERP_BICUBIC, include/xrs.h) against a plain
numpy float64 restatement, bit for bit: the reference uses no transcendental
and the kernel's operation order."""

from __future__ import annotations

import dataclasses
import math

import numpy as np
import pytest

from helpers import assert_bitwise_equal
from oracle import reproject_ref


def _axis(s, origin, res, win, w0, size):
    """(inside, four clamped global tap indices, four weights) along one axis."""
    i = (s - np.float64(origin)) / res
    fl, ce = np.floor(i).astype(np.int16), np.ceil(i).astype(np.int16)
    d = i - fl
    idx = []
    for w in (fl.astype(np.int64), ce.astype(np.int64)):
        w = np.where(w < 0, w + win, w)
        assert ((w >= 0) & (w < win)).all()
        idx.append(np.where((w0 + w >= 0) & (w0 + w < size), w0 + w, -1))
    taps = [np.clip(idx[0] - 1 + k, 0, size - 1) for k in range(4)]
    wts = [((-0.5 * d + 1.0) * d - 0.5) * d, (1.5 * d - 2.5) * (d * d) + 1.0,
           ((-1.5 * d + 2.0) * d + 0.5) * d, (0.5 * d - 0.5) * (d * d)]
    return (idx[0] >= 0) & (idx[1] >= 0), taps, wts


def bicubic_ref(data, sgm, tgm, transform_bounds, sxx, syy, fill):
    """Bicubic of (n, H, W) `data` at the source-CRS positions (sxx, syy) of
    the target pixels; tile windows and float32 origins from the oracle."""
    n, h, w = data.shape
    tw, th = tgm.tile_size
    ntx, nty = math.ceil(tgm.width / tw), math.ceil(tgm.height / th)
    b, xc, yc, pad = reproject_ref.get_scr_bboxes_indices(
        transform_bounds, sgm.x_coords.values, sgm.y_coords.values, sgm.x_res, sgm.y_res, w, h,
        tgm.xy_bboxes, ntx, nty)
    v = data.astype(np.float64)
    out = np.empty((n, tgm.height, tgm.width), np.float64)
    for j in range(nty):
        for i in range(ntx):
            sl = np.s_[j * th:(j + 1) * th, i * tw:(i + 1) * tw]
            okx, tx, wx = _axis(sxx[sl], xc[0, j, i], sgm.x_res, xc.shape[0],
                                int(b[0, j, i]) - pad[2][0], w)
            oky, ty, wy = _axis(syy[sl], yc[0, j, i], -sgm.y_res, yc.shape[0],
                                int(b[1, j, i]) - pad[1][0], h)
            hh = [((wx[0] * v[:, r, tx[0]] + wx[1] * v[:, r, tx[1]]) + wx[2] * v[:, r, tx[2]])
                  + wx[3] * v[:, r, tx[3]] for r in ty]
            res = ((wy[0] * hh[0] + wy[1] * hh[1]) + wy[2] * hh[2]) + wy[3] * hh[3]
            out[(slice(None),) + sl] = np.where(okx & oky, res, fill)
    return out


def test_reference_pins_itself():
    """d = 0 returns the source; a cubic polynomial is reproduced exactly at
    interior half-pixel positions (the weights are (-1, 9, 9, -1) / 16: exact
    for cubics per axis, and every product of these dyadic values is exact)."""
    import xcube_resampling_amd as xrs

    sgm = xrs.GridMapping.regular((5, 5), (0, 0), 1.0, "EPSG:4326")
    xs, ys = sgm.x_coords.values, sgm.y_coords.values
    data = np.arange(25, dtype=np.float64).reshape(1, 5, 5) ** 2
    tgm = xrs.GridMapping.regular((5, 5), (0, 0), 1.0, "EPSG:4326", tile_size=(5, 5))
    xx, yy = np.meshgrid(xs, ys)
    assert_bitwise_equal(bicubic_ref(data, sgm, tgm, lambda *b: b, xx, yy, np.nan), data)
    cubic = lambda x, y: x * x * x - 2.0 * x * y * y + y   # noqa: E731
    tgm = xrs.GridMapping.regular((2, 2), (1.5, 1.5), 1.0, "EPSG:4326", tile_size=(2, 2))
    hx, hy = np.meshgrid(tgm.x_coords.values, tgm.y_coords.values)   # half-pixel positions
    assert_bitwise_equal(bicubic_ref(cubic(xx, yy)[None], sgm, tgm, lambda *b: b, hx, hy, np.nan),
                         cubic(hx, hy)[None])


def _case(ssize, smin, sres, scrs, tsize, tmin, tres, tcrs, ttile, dtype, n=1, seed=3):
    import xcube_resampling_amd as xrs
    from xcube_resampling_amd.crs import Transformer
    from xcube_resampling_amd.reproject import plan_reproject

    sgm = xrs.GridMapping.regular(ssize, smin, sres, scrs)
    tgm = xrs.GridMapping.regular(tsize, tmin, tres, tcrs, tile_size=ttile)
    tr = Transformer.from_crs(tgm.crs, sgm.crs, always_xy=True)
    plan = plan_reproject(sgm, tgm, tr)
    sx, sy = plan.host_coords()
    if sx.ndim == 1:
        sx, sy = np.meshgrid(sx, sy)
    else:   # the position tables are an input of the comparison, not its subject
        plan = dataclasses.replace(plan, src_x=sx, src_y=sy, _device_cache={})
    rng = np.random.default_rng(seed)
    shape = (n, ssize[1], ssize[0])
    data = (rng.random(shape) * 200).astype(dtype) if np.dtype(dtype).kind in "iu" else \
        rng.standard_normal(shape).astype(dtype)
    return sgm, tgm, tr, plan, sx, sy, data


def _run(plan, data, fill=np.nan, band=None, **kw):
    import torch
    from xcube_resampling_amd import _native, kernels

    src = torch.from_numpy(data).cuda()
    if band is None:
        return kernels.reproject(src, plan, "bicubic", fill, **kw).cpu().numpy()
    with _native.testing_knob("reproject_band", band):
        return kernels.reproject(src, plan, "bicubic", fill, **kw).cpu().numpy()


# EPSG:4326 -> EPSG:3857 over 1-74 N: the source-row step per target row falls
# from 1.2 to 0.3; one 512-column segment plus a remainder, three tile rows
MERC = ((700, 80), (-14.0, 0.0), (0.04, 0.9375), "EPSG:4326",
        (549, 100), (-1050000.0, 111325.0), (4000.0, 124000.0), "EPSG:3857", (600, 48))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("dtype,out", [("float32", "float64"), ("float32", "float32"),
                                       ("float64", "float64"), ("int16", "float64"),
                                       ("uint8", "float64")])
def test_separable_mercator(dtype, out, n):
    sgm, tgm, tr, plan, sx, sy, data = _case(*MERC, dtype, n)
    ref = bicubic_ref(data, sgm, tgm, tr.transform_bounds, sx, sy, np.nan).astype(out)
    assert np.isfinite(ref).all()
    assert_bitwise_equal(_run(plan, data, out_dtype=np.dtype(out)), ref)
    # bands of 5 rows split the tiles: the ring restarts in mid-tile
    assert_bitwise_equal(_run(plan, data, band=5, out_dtype=np.dtype(out)), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("name,args,fill", [
    # x3 upsampling on dyadic grids: the ring serves rows without advancing
    ("up", ((40, 30), (8, 4), 0.5, "EPSG:4326", (150, 110), (8, 4), 0.125, "EPSG:4326",
            (64, 48)), np.nan),
    # row step 5: every target row refills the ring; step 3: partial refills
    ("down5", ((300, 300), (0, 0), 0.25, "EPSG:4326", (58, 57), (1, 1), 1.25, "EPSG:4326",
               (32, 40)), np.nan),
    ("down3", ((300, 300), (0, 0), 0.25, "EPSG:4326", (90, 90), (1, 1), 0.75, "EPSG:4326",
               (64, 50)), np.nan),
    # the target reaches two pixels beyond the source on every side
    ("edge_nan", ((30, 20), (10, 40), 0.5, "EPSG:4326", (34, 24), (9, 39), 0.5, "EPSG:4326",
                  (20, 16)), np.nan),
    ("edge_int", ((30, 20), (10, 40), 0.5, "EPSG:4326", (76, 56), (9.5, 39.5), 0.21,
                  "EPSG:4326", (40, 30)), -7.0),
])
def test_identity_crs_cases(name, args, fill):
    dtype = "int16" if name == "edge_int" else "float32"
    sgm, tgm, tr, plan, sx, sy, data = _case(*args, dtype)
    if name == "edge_nan":
        data[0, 7, 11] = np.nan
    ref = bicubic_ref(data, sgm, tgm, tr.transform_bounds, sx, sy, fill)
    got = _run(plan, data, fill)
    assert_bitwise_equal(got, ref)
    if name.startswith("edge"):
        border = np.ones(got.shape[1:], bool)
        border[2:-2, 2:-2] = False
        assert_bitwise_equal(got[0][border], np.full(int(border.sum()), fill))
    if name == "edge_nan":   # the NaN reaches exactly the pixels whose 4 x 4 footprint holds it
        inner = np.isnan(got[0, 2:-2, 2:-2])
        assert inner.sum() == 16 and inner[5:9, 9:13].all()


@pytest.mark.gpu
@pytest.mark.parametrize("tsize,ttile", [((5, 5), (5, 5)), ((10, 10), (4, 6))])
def test_non_separable_utm_to_laea(tsize, ttile):
    args = ((5, 5), (565250.0, 5933850.0), 100.0, "EPSG:32632",
            tsize, (4320080, 3382480), 400 // tsize[0], "epsg:3035", ttile)
    sgm, tgm, tr, plan, sx, sy, data = _case(*args, "float32", 2)
    assert plan.coord_mode == 1 and not plan.fused_transform("cuda:0", "bicubic")
    ref = bicubic_ref(data, sgm, tgm, tr.transform_bounds, sx, sy, np.nan)
    assert np.isfinite(ref).any()
    assert_bitwise_equal(_run(plan, data), ref)


@pytest.mark.gpu
def test_banded_paths_equal_the_single_launch():
    import xcube_resampling_amd as xrs
    from xcube_resampling_amd import streaming
    from xcube_resampling_amd.reproject import _reproject_partitioned

    sgm, tgm, tr, plan, sx, sy, data = _case(*MERC, "float32", 2)
    whole = _run(plan, data)
    assert_bitwise_equal(_reproject_partitioned(data, plan, "bicubic", np.nan, None,
                                                ["cuda:0", "cuda:0"]), whole)
    assert_bitwise_equal(streaming.reproject_host(data, plan, "bicubic", np.nan, band_rows=24),
                         whole)
    r0, r1 = 37, 71   # a row band with exactly its halo rows resident
    j0, j1 = plan.source_rows_read(r0, r1, halo=1)
    assert (j0, j1) != plan.source_rows_read(r0, r1)
    part = _run(plan, np.ascontiguousarray(data[:, j0:j1]), rows=(r0, r1), src_row0=j0)
    assert_bitwise_equal(part, whole[:, r0:r1])
    lon, lat = sgm.x_coords.values, sgm.y_coords.values
    ds = xrs.Dataset(data_vars={"a": (("t", "lat", "lon"), data), "b": (("t", "lat", "lon"), data)},
                     coords={"lon": ("lon", lon), "lat": ("lat", lat)})
    out = xrs.reproject_dataset(ds, tgm, interp_methods={"a": "bicubic", "b": "bilinear"})
    assert_bitwise_equal(out["a"].values, whole)
    assert not np.array_equal(out["b"].values, whole)
    assert_bitwise_equal(xrs.reproject_dataset(ds, tgm, interp_methods="bicubic")["b"].values, whole)
