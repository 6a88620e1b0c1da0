"""GPU tests of K8 (xrs_coords_stats) and the device path of
GridMapping.from_coords built on it.

Reference: the numpy code of xcube_resampling_amd/gridmapping/coords.py (the
float64 restatement of coords.py:99-327 pinned by the reference goldens),
called directly / with the host path forced.

Projected mode is IEEE-identical to numpy (add, multiply, square root, no
contraction): values and indices are compared exactly.  Geographic mode differs
by the device cosine: tests/test_transform_gpu.py bounds device libm against
numpy by RTOL = 1e-12 relative; the area is that cosine times exactly computed
factors through two further products, so numpy's area at K8's index lies within
COS_MARGIN = 1e-12 + 2 * 2**-53 (relative) of numpy's extreme.  The swaths
below keep their two smallest and two largest areas > 1e-7 apart (checked per
case), so K8's index must equal numpy's there too."""

from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS_MARGIN = 1e-12 + 2 * 2.0**-53
MIN_GAP = 1e-7   # relative gap of the two smallest / largest areas of the swaths


def swath(h, w, geographic, seed=5):
    """A smoothly warped (h, w) swath: lon / lat degrees or metres."""
    a = np.random.default_rng(seed).uniform(0.5, 1.5, 4)
    jj, ii = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64),
                         indexing="ij")
    u = ii + 0.2 * jj + 0.03 * a[0] * ii * ii / w + 1.5 * np.sin(a[1] + 0.11 * ii + 0.07 * jj)
    v = jj - 0.15 * ii + 0.02 * a[2] * jj * jj / h + 1.2 * np.cos(a[3] + 0.05 * ii + 0.13 * jj)
    if geographic:
        return 10.0 + 0.02 * u, 60.0 - 0.015 * v
    return 4.0e6 + 300.0 * u, 3.0e6 - 250.0 * v


def crs_of(geographic):
    from xcube_resampling_amd.crs import normalize_crs
    return normalize_crs("EPSG:4326" if geographic else "EPSG:3035")


def device_view(a, pad=0):
    """`a` on the device; pad > 0: as a row-strided view of a wider tensor."""
    import torch
    if not pad:
        return torch.from_numpy(a).cuda()
    wide = torch.full((a.shape[0], a.shape[1] + 2 * pad), float("nan"), dtype=torch.float64,
                      device="cuda")
    wide[:, pad:pad + a.shape[1]] = torch.from_numpy(a).cuda()
    return wide[:, pad:pad + a.shape[1]]


def check_against_numpy(x, y, geographic, pad=0):
    from xcube_resampling_amd import kernels
    from xcube_resampling_amd.gridmapping import coords

    ref = coords._positive_areas(x, y, crs_of(geographic))
    st = kernels.coords_stats(device_view(x, pad), device_view(y, pad), geographic)
    assert st.n_positive == np.count_nonzero(~np.isnan(ref))
    assert st.any_gt_180 == bool(np.any(x > 180))
    imin, imax = int(np.nanargmin(ref)), int(np.nanargmax(ref))
    if not geographic:
        assert (st.idx_min, st.idx_max) == (imin, imax)
        assert (st.area_min, st.area_max) == (ref[imin], ref[imax])   # bit for bit
        return
    assert abs(ref[st.idx_min] - ref[imin]) <= COS_MARGIN * ref[imin]
    assert abs(ref[st.idx_max] - ref[imax]) <= COS_MARGIN * ref[imax]
    assert st.area_min == pytest.approx(ref[imin], rel=COS_MARGIN, abs=0)
    assert st.area_max == pytest.approx(ref[imax], rel=COS_MARGIN, abs=0)
    s = np.sort(ref[~np.isnan(ref)])
    assert s[1] - s[0] > MIN_GAP * s[0] and s[-1] - s[-2] > MIN_GAP * s[-1]
    assert (st.idx_min, st.idx_max) == (imin, imax)


# (2, 2); a lane-63 neighbour across a column block; a row halo across a
# 16-row block; several blocks both ways; a row-strided view
@pytest.mark.parametrize("geographic", [False, True], ids=["projected", "geographic"])
@pytest.mark.parametrize("h,w,pad", [(2, 2, 0), (3, 65, 0), (17, 64, 0), (33, 130, 0),
                                     (40, 200, 28)])
def test_kernel_matches_numpy(h, w, pad, geographic):
    x, y = swath(h, w, geographic)
    check_against_numpy(x, y, geographic, pad)


def _tie(x, y):        # two equal minimum (2 sqrt(2.5)) and maximum (5) areas, the rest 4
    jj, ii = np.meshgrid(np.arange(x.shape[0]), np.arange(x.shape[1]), indexing="ij")
    x[...], y[...] = 2.0 * ii, -2.0 * jj
    x[5, 40] += 0.5
    x[18, 66] += 0.5


def _nan(x, y):
    x[7, 9] = np.nan
    y[16, 63] = np.nan


def _repeat(x, y):     # differences of 0 and of ~5e-9 (<= 1e-8) count as 0
    x[3, 5], y[3, 5] = x[3, 4], y[3, 4]
    x[16, 64], y[16, 64] = x[16, 63] + 5e-9, y[16, 63]


def _inf(x, y):
    x[2, 3] = np.inf
    y[19, 69] = -np.inf


def _over_180(x, y):    # the single value above 180: the last point
    x[...] = 100.0 + 79.0 * (x - x.min()) / (x.max() - x.min())
    x[-1, -1] = 180.0000001


def _degenerate(x, y):  # every area 0, the coordinates not regular
    y[...] = 3.0e6


@pytest.mark.parametrize("plant", [_tie, _nan, _repeat, _inf, _over_180, _degenerate])
def test_planted_cases(plant):
    import xcube_resampling_amd as xrs
    from xcube_resampling_amd import kernels

    x, y = swath(20, 70, False)
    plant(x, y)
    if plant is not _degenerate:
        check_against_numpy(x, y, False)
        return
    st = kernels.coords_stats(device_view(x), device_view(y), False)
    assert (st.n_positive, st.idx_min, st.idx_max) == (0, -1, -1)
    assert np.isnan(st.area_min) and np.isnan(st.area_max)
    for data in ((x, y), (device_view(x), device_view(y))):   # numpy's error, both paths
        with pytest.raises(ValueError, match="All-NaN slice encountered"):
            xrs.GridMapping.from_coords(xrs.DataArray(data[0], ("y", "x")),
                                        xrs.DataArray(data[1], ("y", "x")), "EPSG:3035")


GM_FIELDS = ("xy_res", "xy_bbox", "is_regular", "is_lon_360", "is_j_axis_up", "size")


@pytest.mark.parametrize("geographic", [False, True], ids=["projected", "geographic"])
def test_from_coords_device_equals_numpy(geographic):
    import xcube_resampling_amd as xrs

    x, y = swath(130, 200, geographic)
    crs = "EPSG:4326" if geographic else "EPSG:3035"
    with xrs.set_options(coords_device_min_points=1 << 60):   # host path forced
        ref = xrs.GridMapping.from_coords(xrs.DataArray(x, ("y", "x")),
                                          xrs.DataArray(y, ("y", "x")), crs)
    for min_points, data in ((1 << 60, (device_view(x), device_view(y))), (0, (x, y))):
        with xrs.set_options(coords_device_min_points=min_points):
            gm = xrs.GridMapping.from_coords(xrs.DataArray(data[0], ("y", "x")),
                                             xrs.DataArray(data[1], ("y", "x")), crs)
        assert gm.x_coords.data.is_cuda   # device tensors kept, an upload handed on
        for f in GM_FIELDS:
            assert getattr(gm, f) == getattr(ref, f), f


@pytest.mark.parametrize("target_crs", ["EPSG:4326", "EPSG:3035"])
def test_rectify_with_device_coordinates_equals_numpy(target_crs):
    """EPSG:3035: the coordinates pass through _transform_coords on the device."""
    import torch

    import xcube_resampling_amd as xrs

    lon, lat = swath(130, 200, True)
    v = np.random.default_rng(1).random((130, 200), dtype=np.float32)

    def dataset(to_dev):
        return xrs.Dataset(data_vars={"v": (("y", "x"), torch.from_numpy(v).cuda())},
                           coords={"lon": (("y", "x"), to_dev(lon)),
                                   "lat": (("y", "x"), to_dev(lat))})

    with xrs.set_options(coords_device_min_points=1 << 60):   # host path forced
        gm = xrs.GridMapping.from_dataset(dataset(np.asarray))
        tgm = gm.transform(target_crs).to_regular() if target_crs != "EPSG:4326" else None
        ref = xrs.rectify_dataset(dataset(np.asarray), target_gm=tgm)["v"].values
    out = xrs.rectify_dataset(dataset(device_view), target_gm=tgm)["v"].values
    assert np.isfinite(ref).mean() > 0.5
    assert out.dtype == ref.dtype and np.array_equal(out, ref, equal_nan=True)
