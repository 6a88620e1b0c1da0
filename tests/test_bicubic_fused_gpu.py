"""Bicubic with the projection fused into the gather (K1pq: xrs_reproject_proj,
XRS_INTERP_BICUBIC) against test_bicubic_gpu's numpy float64 restatement, bit
for bit.  The reference is evaluated at the positions xrs_transform returns on
the device: they are an input of the comparison, not its subject."""

from __future__ import annotations

import dataclasses
import functools

import numpy as np
import pytest

from helpers import assert_bitwise_equal
from test_bicubic_gpu import _case, bicubic_ref

pytestmark = pytest.mark.gpu

UTM = ((900, 700), (400000.0, 5500000.0), 100.0, "EPSG:32632")
# name: (_case arguments, elements of a staging budget that one launch's 32 x 8
# patches straddle).  The LAEA targets start where the UTM source lies, so the
# reference is finite on more than half the pixels (checked below).
GEOMS = {
    # two steps near 1:1: every rectangle (39 x 12 or 39 x 13 elements) fits
    "near": (UTM + ((800, 640), (4150000.0, 2951000.0), 110.0, "EPSG:3035", (256, 192)), 480),
    # 5 x coarser: 175 x 45 elements, beyond the default budget for float64
    "coarse": (UTM + ((160, 128), (4150000.0, 2951000.0), 550.0, "EPSG:3035", (64, 48)), 7800),
    # 12 x coarser: 415 x 102, beyond it for every dtype; edge patches still fit
    "coarse12": (UTM + ((66, 53), (4150000.0, 2951000.0), 1320.0, "EPSG:3035", (24, 20)), 8000),
    # width and tiles no multiple of the patch (451 patches straddle tiles), 60
    # pixels beyond the source on every side: fill, edge taps, 555 empty patches
    "ragged": (UTM + ((733, 595), (4140000.0, 2941000.0), 150.0, "EPSG:3035", (100, 75)), 780),
    # one step (tmerc inverse): geographic source onto a UTM target
    "onestep": (((600, 500), (8.0, 49.0), 0.001, "EPSG:4326",
                 (480, 560), (430000.0, 5432000.0), 80.0, "EPSG:32632", (200, 160)), 360),
}
DTYPES = [("float32", "float64"), ("float32", "float32"), ("float64", "float64"),
          ("int16", "float64"), ("uint8", "float64")]


@functools.lru_cache(maxsize=None)
def _geom(name):
    """(sgm, tgm, tr, plain plan, device positions on the host) of a geometry."""
    from xcube_resampling_amd import kernels
    from xcube_resampling_amd.reproject import plan_reproject

    sgm, tgm, tr, _, _, _, _ = _case(*GEOMS[name][0], "uint8")
    plan = plan_reproject(sgm, tgm, tr)
    assert plan.coord_mode == 1 and plan.src_x is None
    sx, sy = kernels.transform(plan.transformer, plan.grid_x, plan.grid_y, True)
    return sgm, tgm, tr, plan, sx.cpu().numpy(), sy.cpu().numpy()


def _data(name, dtype):
    """Two slices of the geometry's source raster (seeded; ints in [0, 200))."""
    (w, h), rng = GEOMS[name][0][0], np.random.default_rng(3)
    return (rng.random((2, h, w)) * 200).astype(dtype) if np.dtype(dtype).kind in "iu" else \
        rng.standard_normal((2, h, w)).astype(dtype)


def _fused(plan):
    return dataclasses.replace(plan, fuse_transform=True, _device_cache={})


def _run(plan, data, knob=("reproject_proj_bicubic_direct", 0), **kw):
    import torch
    from xcube_resampling_amd import _native, kernels

    src = torch.from_numpy(data).cuda()
    with _native.testing_knob(*knob):
        out = kernels.reproject(src, plan, "bicubic", np.nan, **kw).cpu().numpy()
    return out


@pytest.mark.parametrize("dtype,out", DTYPES)
@pytest.mark.parametrize("name", list(GEOMS))
def test_fused_kernel_against_reference(name, dtype, out):
    sgm, tgm, tr, plan, sx, sy = _geom(name)
    data = _data(name, dtype)
    if data.dtype.kind == "f":
        data[1, data.shape[1] // 2, data.shape[2] // 2] = np.nan
    ref = bicubic_ref(data, sgm, tgm, tr.transform_bounds, sx, sy, np.nan).astype(out)
    assert np.isfinite(ref).mean() > 0.5
    fused, kw = _fused(plan), dict(out_dtype=np.dtype(out))
    mixed = GEOMS[name][1] * data.dtype.itemsize
    # the product's launch, a 32 KiB budget (the design's: coarse rectangles fall
    # back by themselves), every patch forced to global memory under that budget,
    # and a budget that one launch's patches straddle
    for knob in (("reproject_proj_bicubic_lds", 0), ("reproject_proj_bicubic_lds", 32768),
                 ("reproject_proj_bicubic_direct", 1), ("reproject_proj_bicubic_lds", mixed)):
        assert_bitwise_equal(_run(fused, data, knob, **kw), ref)
        assert "cuda:0" not in fused._device_cache   # no coordinate tables were made
    r0, r1 = tgm.height // 3, min(tgm.height // 3 + 43, tgm.height)   # a band, its halo rows
    j0, j1 = plan.source_rows_read(r0, r1, halo=1)
    part = _run(fused, np.ascontiguousarray(data[:, j0:j1]), rows=(r0, r1), src_row0=j0, **kw)
    assert_bitwise_equal(part, ref[:, r0:r1])
    assert "cuda:0" not in fused._device_cache


def test_fused_equals_the_tables_path():
    plan = _geom("near")[3]
    data = _data("near", "float32")
    fused, plain = _fused(plan), dataclasses.replace(plan, _device_cache={})
    assert fused.fused_transform("cuda:0", "bicubic")
    assert not plain.fused_transform("cuda:0", "bicubic")
    whole = _run(plain, data)
    assert "cuda:0" in plain._device_cache and np.isfinite(whole).mean() > 0.5
    assert_bitwise_equal(_run(fused, data), whole)
    r0, r1 = 150, 260
    j0, j1 = plan.source_rows_read(r0, r1, halo=1)
    band = np.ascontiguousarray(data[:, j0:j1])
    assert_bitwise_equal(_run(fused, band, rows=(r0, r1), src_row0=j0), whole[:, r0:r1])
    assert_bitwise_equal(_run(plain, band, rows=(r0, r1), src_row0=j0), whole[:, r0:r1])


@pytest.mark.parametrize("route", ["device", "host_bands", "devices"])
def test_reproject_dataset_honours_the_table_budget(route, monkeypatch):
    import torch

    import xcube_resampling_amd as xrs
    from xcube_resampling_amd import kernels

    sgm, tgm = _geom("ragged")[:2]
    a = _data("ragged", "float32")
    put = (lambda v: torch.from_numpy(v).cuda()) if route == "device" else (lambda v: v)
    ds = xrs.Dataset(data_vars={"v": (("t", "y", "x"), put(a)),
                                "w": (("t", "y", "x"), put(a[::-1].copy()))},
                     coords={"x": ("x", sgm.x_coords.values), "y": ("y", sgm.y_coords.values)})
    opts = {"host_bands": dict(host_streaming_min_bytes=0),
            "devices": dict(devices=["cuda:0", "cuda:0"])}.get(route, {})
    calls, orig = [], kernels._reproject_proj
    monkeypatch.setattr(kernels, "_reproject_proj",
                        lambda *args, **kw: calls.append(args[3]) or orig(*args, **kw))

    def run():
        out = xrs.reproject_dataset(ds, tgm, source_gm=sgm, interp_methods="bicubic")
        return [out[k].values for k in "vw"]

    with xrs.set_options(**opts):
        ref = run()
        assert not calls   # two variables share the tables by default
        with xrs.set_options(reproject_table_max_bytes=0):
            got = run()
    assert len(calls) >= 2 and set(calls) == {3}   # both variables, the bicubic code
    assert np.isfinite(ref[0]).mean() > 0.5 and not np.array_equal(ref[0], ref[1], equal_nan=True)
    for g, r in zip(got, ref):
        assert_bitwise_equal(g, r)


def test_empty_band_raises_on_the_fused_path():
    import torch
    from xcube_resampling_amd import _native, kernels

    plan = _geom("near")[3]
    rows = (40, 100)
    j0, j1 = plan.source_rows_for(*rows, 1)
    assert j1 > j0
    band = torch.zeros((1, 0, 900), dtype=torch.float32, device="cuda")
    fused = _fused(plan)
    with pytest.raises(_native.NativeLibraryError, match="source band"):
        kernels.reproject(band, fused, "bicubic", 0.0, rows=rows, src_row0=j0)
    assert str(band.device) not in fused._device_cache
