"""The polar stereographic and rotated-pole steps on the device: xrs_transform
against numpy under tests/test_transform_gpu.py's criteria, the fused gathers
against the tables path bit for bit, the API against host-made coordinates."""
import dataclasses

import numpy as np
import pytest
from test_transform_gpu import ATOL, RTOL, _grid

pytestmark = pytest.mark.gpu

ROTATED = "rotated"   # the CORDEX EUR-11 pole


def _crs(name):
    import xcube_resampling_amd as xrs
    from xcube_resampling_amd.crs import rotated_pole_crs

    return rotated_pole_crs(39.25, -162.0) if name == ROTATED else xrs.CRS.from_user_input(name)


def _axes(name, n=257):
    """A grid over the CRS's area of use and beyond it."""
    if name == ROTATED:   # EUR-11 spans -28..18 x -23..22 rotated degrees
        return np.linspace(-60.0, 60.0, n), np.linspace(-45.0, 45.0, n)
    if name in ("EPSG:3413", "EPSG:3031"):   # 60 deg of latitude lies 3.3e6 m from the pole
        return np.linspace(-4.0e6, 4.0e6, n), np.linspace(-4.0e6, 4.0e6, n)
    return _grid(name, n)


@pytest.mark.parametrize("src,dst", [
    ("EPSG:4326", "EPSG:3413"), ("EPSG:3413", "EPSG:4326"), ("EPSG:3031", "EPSG:32758"),
    ("EPSG:32633", "EPSG:3995"), ("EPSG:3035", "EPSG:3413"), (ROTATED, "EPSG:4326"),
    ("EPSG:4326", ROTATED), (ROTATED, "EPSG:3035"),
])
def test_device_transform_matches_numpy_restatement(src, dst):
    import xcube_resampling_amd as xrs
    from xcube_resampling_amd import kernels

    tr = xrs.Transformer.from_crs(_crs(src), _crs(dst), always_xy=True)
    gx, gy = _axes(src)
    xx, yy = np.meshgrid(gx, gy)
    ex, ey = tr.transform(xx, yy)
    dx, dy = (t.cpu().numpy() for t in kernels.transform(tr, gx, gy, True))
    unit = "deg" if _crs(dst).is_geographic else "m"
    for got, exp in ((dx, ex), (dy, ey)):
        fin = np.isfinite(exp)
        np.testing.assert_array_equal(np.isfinite(got), fin)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(exp))
        assert fin.sum() > 0.2 * fin.size
        np.testing.assert_allclose(got[fin], exp[fin], rtol=RTOL, atol=ATOL[unit])
    ix, iy = (t.cpu().numpy() for t in kernels.transform(tr, xx, yy, False))   # image mode
    np.testing.assert_array_equal(ix, dx)
    np.testing.assert_array_equal(iy, dy)


# a 64 x 48 source and a 70 x 45 target (no multiple of K1pq's 32 x 8 patch or of
# the 32-pixel tile) that reaches beyond the source on every side
PAIRS = {"EPSG:4326": ((-61.0, 62.0), (0.5, 0.4), "EPSG:3413", (-900.0e3, -2700.0e3), 25.0e3),
         ROTATED: ((-16.0, -12.0), (0.5, 0.5), "EPSG:3035", (2.8e6, 1.75e6), 60.0e3)}


def _plan(src):
    import xcube_resampling_amd as xrs

    xy_min, res, dst, txy_min, tres = PAIRS[src]
    sgm = xrs.GridMapping.regular((64, 48), xy_min, res, _crs(src), tile_size=32)
    tgm = xrs.GridMapping.regular((70, 45), txy_min, tres, dst, tile_size=32)
    tr = xrs.Transformer.from_crs(tgm.crs, sgm.crs, always_xy=True)
    return sgm, tgm, xrs.plan_reproject(sgm, tgm, tr)


@pytest.mark.parametrize("src", list(PAIRS))
@pytest.mark.parametrize("interp", ["nearest", "bilinear", "bicubic"])
@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
def test_fused_gather_equals_tables_path(src, interp, dtype):
    import torch

    from xcube_resampling_amd import kernels

    plan = _plan(src)[2]
    assert plan.coord_mode == 1
    fused = dataclasses.replace(plan, fuse_transform=True, _device_cache={})
    data = np.random.default_rng(5).random((2, 48, 64)) * 200 + 1     # no 0: the fill value
    data = torch.from_numpy(data.astype(dtype)).cuda()
    kw = dict(out_dtype=None if interp == "nearest" else np.float64)
    assert fused.fused_transform(data.device, interp) and not plan.fused_transform(data.device, interp)
    got = kernels.reproject(data, fused, interp, 0, **kw).cpu().numpy()
    exp = kernels.reproject(data, plan, interp, 0, **kw).cpu().numpy()
    assert str(data.device) not in fused._device_cache and got.dtype == exp.dtype
    assert 0.02 < (exp == 0).mean() < 0.8        # targets inside and outside the source
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("interp", ["nearest", "bilinear"])
def test_reproject_dataset_onto_polar_grid(interp, monkeypatch):
    """Two variables (one alone is always fused) onto a grid finer than the
    source (no pre-downscaling): tables == fused (budget 0) == host-made tables,
    the last but for a nearest index within the coordinate tolerance of a
    rounding boundary, bilinear to tolerance / resolution (two axes, data < 200)."""
    import torch

    import xcube_resampling_amd as xrs
    from xcube_resampling_amd import kernels

    sgm = _plan("EPSG:4326")[0]
    tgm = xrs.GridMapping.regular((70, 45), (-560.0e3, -2300.0e3), 12.0e3, "EPSG:3413", tile_size=32)
    plan = xrs.plan_reproject(sgm, tgm, xrs.Transformer.from_crs(tgm.crs, sgm.crs, always_xy=True))
    data = (np.random.default_rng(9).random((3, 48, 64)) * 200).astype(np.float32)
    dev = torch.from_numpy(data).cuda()
    ds = xrs.Dataset(data_vars={"v": (("t", "lat", "lon"), dev), "w": (("t", "lat", "lon"), dev * 2)},
                     coords={"lon": ("lon", sgm.x_coords.values), "lat": ("lat", sgm.y_coords.values)})
    calls, orig = [], kernels._reproject_proj
    monkeypatch.setattr(kernels, "_reproject_proj", lambda *a, **kw: calls.append(1) or orig(*a, **kw))
    tabled = xrs.reproject_dataset(ds, tgm, interp_methods=interp)["v"].values
    assert not calls
    with xrs.set_options(reproject_table_max_bytes=0):
        fused = xrs.reproject_dataset(ds, tgm, interp_methods=interp)["v"].values
    assert len(calls) == 2 and np.array_equal(tabled, fused, equal_nan=True)
    assert 0.2 < np.isfinite(tabled).mean() < 1
    hx, hy = plan.host_coords()
    host_plan = dataclasses.replace(plan, src_x=hx, src_y=hy, _device_cache={})
    exp = kernels.reproject(dev, host_plan, interp, np.nan,
                            out_dtype=tabled.dtype.type).cpu().numpy()
    tol = np.array([ATOL["deg"] / 0.5, ATOL["deg"] / 0.4])   # in source pixels
    if interp == "bilinear":
        np.testing.assert_array_equal(np.isnan(tabled), np.isnan(exp))
        np.testing.assert_allclose(tabled, exp, rtol=0, atol=200 * tol.sum(), equal_nan=True)
        return
    # source index coordinates: a rounding boundary lies at a multiple of 0.5
    u = np.stack([(hx + 61.0) / 0.5, (hy - 62.0) / 0.4])
    near = (np.abs(2 * u - np.round(2 * u)) / 2 <= tol[:, None, None]).any(axis=0)
    assert near.mean() <= 0.01
    same = (tabled == exp) | (np.isnan(tabled) & np.isnan(exp))
    assert (same | near).all()


def test_rectify_swath_onto_polar_grid():
    """rectify's device transform of a swath's coordinates (_transform_coords)
    against the same call on coordinates the numpy Transformer made."""
    import xcube_resampling_amd as xrs

    j, i = np.meshgrid(np.arange(40.0), np.arange(50.0), indexing="ij")
    lon, lat = -40.0 + 0.55 * i + 0.21 * j, 82.0 - 0.09 * j - 0.012 * i
    rad = np.random.default_rng(3).random((40, 50))
    tgm = xrs.GridMapping.regular((84, 50), (40.0e3, -1250.0e3), 10.0e3, "EPSG:3413")
    swath = xrs.Dataset(data_vars={"rad": (("y", "x"), rad)},
                        coords={"lon": (("y", "x"), lon), "lat": (("y", "x"), lat)})
    got = xrs.rectify_dataset(swath, target_gm=tgm, interp_methods="bilinear")["rad"].values
    tx, ty = xrs.Transformer.from_crs("EPSG:4326", tgm.crs, always_xy=True).transform(lon, lat)
    moved = xrs.Dataset(data_vars={"rad": (("y", "x"), rad)},
                        coords={"transformed_x": (("y", "x"), tx), "transformed_y": (("y", "x"), ty)})
    sgm = xrs.GridMapping.from_dataset(moved, crs=tgm.crs)
    exp = xrs.rectify_dataset(moved, target_gm=tgm, source_gm=sgm,
                              interp_methods="bilinear")["rad"].values
    assert np.isfinite(exp).mean() > 0.3
    np.testing.assert_array_equal(np.isnan(got), np.isnan(exp))
    # source pixels are > 8 km apart: the coordinate tolerance in source pixels, two axes
    np.testing.assert_allclose(got, exp, rtol=0, atol=2 * ATOL["m"] / 8.0e3, equal_nan=True)
