"""CPU checks around K8 (xrs_coords_stats): the binding, the argument checks,
the ``coords_device_min_points`` option and the host fall-back of the lon-360
rewrite.  Nothing here computes on a device: where the device path must be
entered, the upload and the kernel wrapper are replaced."""

from __future__ import annotations

import ctypes
import types

import numpy as np
import pytest

import xcube_resampling_amd as xrs
from xcube_resampling_amd import _native, kernels
from xcube_resampling_amd.gridmapping import coords

I64, INT, PTR = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p


def test_abi_matches_the_header():
    sig = _native._SIGNATURES
    assert sig["xrs_coords_stats_workspace_size"] == (I64, [I64, I64])
    assert sig["xrs_coords_stats"] == (INT, [PTR, PTR, I64, I64, I64, INT, PTR, PTR, I64, PTR])
    assert ctypes.sizeof(_native.CoordsStats) == 48
    assert _native.CoordsStats.any_gt_180.offset == 40


@pytest.mark.parametrize("h,w,stride,ws_bytes", [
    (1, 8, 8, 1 << 20), (8, 1, 1, 1 << 20),   # h < 2, w < 2
    (8, 8, 7, 1 << 20),                       # row stride below the width
    (8, 8, 8, 47),                            # workspace too small
    (1 << 31, 8, 8, 1 << 20),                 # beyond the 32-bit shape limit
])
def test_argument_errors_before_any_device_work(h, w, stride, ws_bytes):
    lib = _native.load_library()
    fake = PTR(4096)   # never dereferenced: validation fails first
    assert lib.xrs_coords_stats(fake, fake, h, w, stride, 0, fake, fake, ws_bytes,
                                None) == _native.XRS_ERR_ARG
    assert b"xrs_coords_stats" in lib.xrs_last_error()
    # one 48-byte record per block, a multiple of 8 blocks, at most 4096
    assert lib.xrs_coords_stats_workspace_size(8, 8) == 8 * 48
    assert lib.xrs_coords_stats_workspace_size(4000, 4800) == 4096 * 48


def swath(h=40, w=50):
    jj, ii = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64),
                         indexing="ij")
    return 170.0 + 0.4 * ii + 0.05 * jj + 0.3 * np.sin(0.2 * jj), 60.0 - 0.3 * jj - 0.04 * ii


def from_coords(x, y):
    return xrs.GridMapping.from_coords(xrs.DataArray(x, ("y", "x")),
                                       xrs.DataArray(y, ("y", "x")), "EPSG:4326")


class DevicePathEntered(Exception):
    pass


def test_option_decides_which_numpy_arrays_take_the_device_path(monkeypatch):
    import torch

    from xcube_resampling_amd import streaming

    def entered(*a, **k):
        raise DevicePathEntered

    monkeypatch.setattr(kernels, "coords_stats", entered)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(streaming, "host_to_device", lambda a, device: torch.from_numpy(a))
    x, y = swath()
    with xrs.set_options(coords_device_min_points=x.size + 1):   # below: numpy only
        gm = from_coords(x, y)
    assert isinstance(gm.x_coords.data, np.ndarray) and gm.is_lon_360
    with xrs.set_options(coords_device_min_points=x.size):
        with pytest.raises(DevicePathEntered):
            from_coords(x, y)
        # an explicit xy_res skips the estimate and keeps the host path
        coords.new_grid_mapping_from_coords(xrs.DataArray(x, ("y", "x")),
                                            xrs.DataArray(y, ("y", "x")), "EPSG:4326", xy_res=0.3)


def test_lon_360_rewrite_falls_back_to_the_host(monkeypatch):
    import torch

    x, y = swath()
    x = np.where(x > 180, x - 360, x)   # a jump of ~360 degrees along the rows
    ref = from_coords(x, y)
    assert ref.is_lon_360 and not ref.is_regular
    calls = []

    def flag_only(xd, yd, geographic, stream=None):   # any(x > 180) is False here
        calls.append(geographic)
        return types.SimpleNamespace(any_gt_180=False)

    monkeypatch.setattr(kernels, "coords_stats", flag_only)
    monkeypatch.setattr(coords, "_device_coords_2d",
                        lambda xc, yc: (torch.from_numpy(xc.data), torch.from_numpy(yc.data)))
    gm = from_coords(x, y)
    assert calls == [True]   # the estimate ran in numpy, on the rewritten longitudes
    assert isinstance(gm.x_coords.data, np.ndarray) and isinstance(gm.y_coords.data, np.ndarray)
    for f in ("xy_res", "xy_bbox", "is_regular", "is_lon_360", "is_j_axis_up", "size"):
        assert getattr(gm, f) == getattr(ref, f), f
    assert np.array_equal(gm.x_coords.values, ref.x_coords.values)
