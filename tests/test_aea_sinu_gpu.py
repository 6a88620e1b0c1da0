"""The Albers and sinusoidal steps on the device: xrs_transform against numpy under
tests/test_transform_gpu.py's criteria, the fused gathers against the tables path bit
for bit, the API against host-made coordinates, rectify onto an Albers grid."""
import dataclasses

import numpy as np
import pytest
from test_transform_gpu import ATOL, RTOL, _grid

pytestmark = pytest.mark.gpu

MODIS, SINU = "modis", "sinu wgs84"   # the MODIS sphere; an ellipsoidal one about 20 deg E


def _crs(name):
    import xcube_resampling_amd as xrs
    from xcube_resampling_amd.crs import sinusoidal_crs

    if name == MODIS:
        return sinusoidal_crs()
    if name == SINU:
        return sinusoidal_crs(20.0, 6378137.0, 298.257223563)
    return xrs.CRS.from_user_input(name)


def _axes(name, n=257):
    """A grid over the CRS's area of use and beyond it; for the sinusoidal CRSs the
    bounding rectangle of the global map (2 / pi = 0.637 of it lies inside the lobes)."""
    if name == MODIS:
        return np.linspace(-2.0015e7, 2.0015e7, n), np.linspace(-1.0008e7, 1.0008e7, n)
    if name == SINU:
        return np.linspace(-2.0038e7, 2.0038e7, n), np.linspace(-1.0003e7, 1.0003e7, n)
    if name == "EPSG:5070":   # CONUS lies in -2.4e6..2.3e6 x 0.3e6..3.2e6; inside the domain
        return np.linspace(-3.0e6, 3.0e6, n), np.linspace(-1.0e6, 4.0e6, n)
    if name == "EPSG:3413":
        return np.linspace(-4.0e6, 4.0e6, n), np.linspace(-4.0e6, 4.0e6, n)
    return _grid(name, n)


# (source, target, least share of finite results, least share of non-finite results):
# the numpy restatement's shares on the sinusoidal source grids are 0.6313 / 0.3687
# (MODIS) and 0.6310 / 0.3690 (ellipsoidal); every other pair is finite everywhere
@pytest.mark.parametrize("src,dst,finite,nonfinite", [
    ("EPSG:4326", "EPSG:5070", 0.99, 0), ("EPSG:5070", "EPSG:4326", 0.99, 0),
    ("EPSG:4326", MODIS, 0.99, 0), (MODIS, "EPSG:4326", 0.6, 0.3),
    (MODIS, "EPSG:3035", 0.6, 0.3), ("EPSG:32631", "EPSG:3577", 0.99, 0),
    (SINU, "EPSG:5070", 0.6, 0.3), ("EPSG:3413", MODIS, 0.99, 0),
])
def test_device_transform_matches_numpy_restatement(src, dst, finite, nonfinite):
    import xcube_resampling_amd as xrs
    from xcube_resampling_amd import kernels

    tr = xrs.Transformer.from_crs(_crs(src), _crs(dst), always_xy=True)
    gx, gy = _axes(src)
    xx, yy = np.meshgrid(gx, gy)
    with np.errstate(invalid="ignore"):   # the second step's sines of +inf
        ex, ey = tr.transform(xx, yy)
    dx, dy = (t.cpu().numpy() for t in kernels.transform(tr, gx, gy, True))
    unit = "deg" if _crs(dst).is_geographic else "m"
    for got, exp in ((dx, ex), (dy, ey)):
        fin = np.isfinite(exp)
        np.testing.assert_array_equal(np.isfinite(got), fin)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(exp))
        assert fin.mean() >= finite and (~fin).mean() >= nonfinite
        np.testing.assert_allclose(got[fin], exp[fin], rtol=RTOL, atol=ATOL[unit])
    ix, iy = (t.cpu().numpy() for t in kernels.transform(tr, xx, yy, False))   # image mode
    np.testing.assert_array_equal(ix, dx)
    np.testing.assert_array_equal(iy, dy)


# a 64 x 48 source; a 70 x 45 target (no multiple of K1pq's 32 x 8 patch or of the
# 32-pixel tile) that reaches beyond the source, for the sinusoidal source beyond
# lon_0 + 180 too (the far side of the lobes); a finer 70 x 45 target for the API test
PAIRS = {"EPSG:4326": ((-110.0, 30.0), (0.5, 0.4), "EPSG:5070", (-1.2e6, 0.6e6), 40.0e3,
                       (-4.0e5, 2.5e6), 12.0e3),
         MODIS: ((5.0e6, 4.0e6), (100.0e3, 100.0e3), "EPSG:4326", (100.0, 30.0), (1.3, 1.1),
                 (95.0, 45.0), (0.4, 0.4))}


def _plan(src, api=False):
    import xcube_resampling_amd as xrs

    xy_min, res, dst, txy_min, tres, axy_min, ares = PAIRS[src]
    sgm = xrs.GridMapping.regular((64, 48), xy_min, res, _crs(src), tile_size=32)
    tgm = xrs.GridMapping.regular((70, 45), axy_min if api else txy_min, ares if api else tres,
                                  dst, tile_size=32)
    tr = xrs.Transformer.from_crs(tgm.crs, sgm.crs, always_xy=True)
    return sgm, tgm, xrs.plan_reproject(sgm, tgm, tr)


def _outside(src, plan):
    """The target pixels whose numpy-made source coordinates miss the source grid."""
    (x0, y0), (rx, ry) = PAIRS[src][:2]
    hx, hy = plan.host_coords()
    with np.errstate(invalid="ignore"):
        return ~((hx >= x0) & (hx <= x0 + 64 * rx) & (hy >= y0) & (hy <= y0 + 48 * ry))


@pytest.mark.parametrize("src", list(PAIRS))
@pytest.mark.parametrize("interp", ["nearest", "bilinear", "bicubic"])
@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
def test_fused_gather_equals_tables_path(src, interp, dtype):
    import torch

    from xcube_resampling_amd import kernels

    plan = _plan(src)[2]
    assert plan.coord_mode == 1
    assert 0.1 < _outside(src, plan).mean() < 0.6     # 0.13 (Albers), 0.51 (sinusoidal)
    fused = dataclasses.replace(plan, fuse_transform=True, _device_cache={})
    data = np.random.default_rng(5).random((2, 48, 64)) * 200 + 1     # no 0: the fill value
    data = torch.from_numpy(data.astype(dtype)).cuda()
    kw = dict(out_dtype=None if interp == "nearest" else np.float64)
    assert fused.fused_transform(data.device, interp) and not plan.fused_transform(data.device, interp)
    got = kernels.reproject(data, fused, interp, 0, **kw).cpu().numpy()
    exp = kernels.reproject(data, plan, interp, 0, **kw).cpu().numpy()
    assert str(data.device) not in fused._device_cache and got.dtype == exp.dtype
    assert (exp == 0).any() and (exp != 0).mean() > 0.3
    assert np.array_equal(got, exp, equal_nan=True)


@pytest.mark.parametrize("src", list(PAIRS))
@pytest.mark.parametrize("interp", ["nearest", "bilinear"])
def test_reproject_dataset_through_the_api(src, interp, monkeypatch):
    """Two variables (one alone is always fused) onto a grid finer than the
    source: tables == fused (budget 0) == host-made tables, the last but for a
    nearest index within the coordinate tolerance of a rounding boundary (at most
    1 % of the pixels; the numpy restatement alone puts none there on these
    grids), bilinear to tolerance / resolution (two axes, data < 200)."""
    import torch

    import xcube_resampling_amd as xrs
    from xcube_resampling_amd import kernels

    sgm, tgm, plan = _plan(src, api=True)
    (x0, y0), (rx, ry) = PAIRS[src][:2]
    data = (np.random.default_rng(9).random((3, 48, 64)) * 200).astype(np.float32)
    dev = torch.from_numpy(data).cuda()
    x, y = sgm.xy_dim_names
    ds = xrs.Dataset(data_vars={"v": (("t", y, x), dev), "w": (("t", y, x), dev * 2)},
                     coords={x: (x, sgm.x_coords.values), y: (y, sgm.y_coords.values)})
    calls, orig = [], kernels._reproject_proj
    monkeypatch.setattr(kernels, "_reproject_proj", lambda *a, **kw: calls.append(1) or orig(*a, **kw))
    tabled = xrs.reproject_dataset(ds, tgm, source_gm=sgm, interp_methods=interp)["v"].values
    assert not calls
    with xrs.set_options(reproject_table_max_bytes=0):
        fused = xrs.reproject_dataset(ds, tgm, source_gm=sgm, interp_methods=interp)["v"].values
    assert len(calls) == 2 and np.array_equal(tabled, fused, equal_nan=True)
    assert 0.2 < np.isfinite(tabled).mean() < 1
    hx, hy = plan.host_coords()
    host_plan = dataclasses.replace(plan, src_x=hx, src_y=hy, _device_cache={})
    exp = kernels.reproject(dev, host_plan, interp, np.nan,
                            out_dtype=tabled.dtype.type).cpu().numpy()
    unit = "deg" if sgm.crs.is_geographic else "m"
    tol = np.array([ATOL[unit] / rx, ATOL[unit] / ry])   # in source pixels
    if interp == "bilinear":
        np.testing.assert_array_equal(np.isnan(tabled), np.isnan(exp))
        np.testing.assert_allclose(tabled, exp, rtol=0, atol=200 * tol.sum(), equal_nan=True)
        return
    # source index coordinates: a rounding boundary lies at a multiple of 0.5
    with np.errstate(invalid="ignore"):
        u = np.stack([(hx - x0) / rx, (hy - y0) / ry])
        near = (np.abs(2 * u - np.round(2 * u)) / 2 <= tol[:, None, None]).any(axis=0)
    assert near.mean() <= 0.01
    same = (tabled == exp) | (np.isnan(tabled) & np.isnan(exp))
    assert (same | near).all()


def test_rectify_swath_onto_albers_grid():
    """rectify's device transform of a swath's coordinates (_transform_coords)
    against the same call on coordinates the numpy Transformer made."""
    import xcube_resampling_amd as xrs

    j, i = np.meshgrid(np.arange(40.0), np.arange(50.0), indexing="ij")
    lon, lat = -100.0 + 0.2 * i + 0.05 * j, 45.0 - 0.1 * j - 0.01 * i
    rad = np.random.default_rng(3).random((40, 50))
    tgm = xrs.GridMapping.regular((100, 50), (-3.4e5, 1.97e6), 10.0e3, "EPSG:5070")
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
