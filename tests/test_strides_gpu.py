"""Strided sources, storage offsets and `out=` views on every compute entry.

kernels.py forwards `tensor.stride()` as is and the product passes row bands
(`src[:, j0:j1]`) and `out=` views, while every other test hands the kernels
contiguous tensors.  Here the source is a view into a larger tensor — odd row
stride, odd storage offset, a slice stride that is not height x row stride —
whose margin holds a sentinel the payload never holds.  Each case asserts
that the result is bitwise the one of `src.contiguous()`, that the same call
into an `out=` view of a sentinel-filled larger tensor gives it too, and that
every margin element of that tensor still holds the sentinel afterwards (the
margin lies inside the allocation: a stray write lands there and is seen).
"""

from __future__ import annotations

import numpy as np
import pytest

from helpers import assert_bitwise_equal

pytestmark = pytest.mark.gpu

INT_SENTINEL = 233   # integer payloads stay below 200


def _sentinel(tdtype):
    return float("nan") if tdtype.is_floating_point else INT_SENTINEL


def embed_shape(shape, contiguous_rows=False):
    """(big shape, row, column) of the view big[1:, row:row+h, col:col+w]:
    one spare leading slice, 4 spare rows, 5 spare columns (6 where that
    makes the row stride odd), placed so that the storage offset is odd."""
    n, h, w = shape
    if contiguous_rows:   # for an `out=` that must keep its rows dense
        return (n + 1, h + 4, w), 2, 0
    pc = 5 if (w + 5) % 2 else 6
    col = 3 if ((h + 6) * (w + pc) + 3) % 2 else 2
    return (n + 1, h + 4, w + pc), 2, col


def embed(payload, contiguous_rows=False):
    """(big, view): `payload` (host array or device tensor, (n, h, w)) as a
    view into a larger sentinel-filled device tensor."""
    import torch

    t = torch.from_numpy(payload) if isinstance(payload, np.ndarray) else payload
    n, h, w = t.shape
    shape, r, c = embed_shape((n, h, w), contiguous_rows)
    big = torch.full(shape, _sentinel(t.dtype), dtype=t.dtype, device="cuda")
    view = big[1:, r:r + h, c:c + w]
    view.copy_(t)
    if not contiguous_rows:
        assert view.stride(1) % 2 == 1 and view.storage_offset() % 2 == 1
        assert view.stride(0) != h * view.stride(1) and view.stride(2) == 1
    return big, view


def empty_view(shape, tdtype, contiguous_rows=False):
    """(big, view): an `out=` view of `shape` in a sentinel-filled tensor."""
    import torch

    bshape, r, c = embed_shape(shape, contiguous_rows)
    big = torch.full(bshape, _sentinel(tdtype), dtype=tdtype, device="cuda")
    return big, big[1:, r:r + shape[1], c:c + shape[2]]


def assert_margin_intact(big, view, msg):
    import torch

    inside = torch.zeros(big.shape, dtype=torch.bool, device=big.device)
    off = view.storage_offset() - big.storage_offset()
    n0, rem = divmod(off, big.stride(0))
    r0, c0 = divmod(rem, big.stride(1))
    inside[n0:n0 + view.shape[0], r0:r0 + view.shape[1], c0:c0 + view.shape[2]] = True
    margin = big[~inside]
    ok = torch.isnan(margin) if big.dtype.is_floating_point else margin == INT_SENTINEL
    assert margin.numel() > 0 and bool(ok.all()), \
        f"{msg}: {int((~ok).sum())} margin elements of the out= tensor were overwritten"


def check(call, payload, msg, out_rows_dense=False, has_out=True):
    """call(src, out) -> device result.  Strided source == contiguous source;
    `out=` view == the same, margins intact."""
    _, view = embed(payload)
    want = call(view.contiguous(), None)
    got = call(view, None)
    assert_bitwise_equal(got.cpu().numpy(), want.cpu().numpy(), f"{msg}: strided source")
    if has_out:
        big, out = empty_view(tuple(want.shape), want.dtype, out_rows_dense)
        res = call(view, out)
        assert res.data_ptr() == out.data_ptr()
        assert_bitwise_equal(out.cpu().numpy(), want.cpu().numpy(), f"{msg}: out= view")
        assert_margin_intact(big, out, msg)
    return want


def _payload(dtype, shape, seed=0):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).kind == "u":
        return rng.integers(0, 200, shape).astype(dtype)
    return rng.standard_normal(shape).astype(dtype)


# ------------------------------------------------------------------ K1 -------
@pytest.mark.parametrize("dtype", ["float32", "uint8", "float64"])
@pytest.mark.parametrize("interp", ["nearest", "bilinear", "bicubic"])
def test_reproject_strided(interp, dtype):
    """96 x 80 -> 150 x 70 in 64 x 48 tiles (test_dtypes_gpu's geometry);
    bicubic on test_bicubic_gpu's Mercator geometry (one 512-column segment
    plus a remainder)."""
    from xcube_resampling_amd import kernels

    if interp == "bicubic":
        from test_bicubic_gpu import MERC, _case
        _, _, _, plan, _, _, data = _case(*MERC, dtype, 2)
    else:
        from test_dtypes_gpu import K1_H, K1_W, _k1_plans
        plan, data = _k1_plans()["gen"], _payload(dtype, (2, K1_H, K1_W))
    fill = 7.0 if dtype == "uint8" else float("nan")
    want = check(lambda s, o: kernels.reproject(s, plan, interp, fill, out=o), data,
                 f"{interp} {dtype}")
    assert np.dtype(str(want.dtype).replace("torch.", "")) == \
        (np.float64 if interp != "nearest" else np.dtype(dtype))


# ------------------------------------------------------------- K2 / K3 -------
def _affine_plan(name, dtype):
    """(plan, source shape) of the named affine case, two slices each."""
    import xcube_resampling_amd.affine as A

    cval = 7 if np.dtype(dtype).kind == "u" else np.nan
    if name == "bicubic":
        from test_affine_bicubic_gpu import GEOMETRIES, _plan
        scale, offset, shape = GEOMETRIES[0]
        return _plan((2,) + shape, dtype, scale, offset, (150, 200), (64, 48), cval), (2,) + shape
    sc, (ox, oy), oshape, tile, agg = {
        "plain": (0.5, (0.25, 0.4), (150, 200), (64, 48), "first"),
        "k3i": (4.0, (0.0, 0.0), (20, 300), (8, 128), "mean"),
        "k3w": (4.0, (0.5, 0.25), (40, 60), (20, 60), "mean"),
        "generic": (2.5, (1.1, -0.4), (30, 50), (30, 25), "max"),
    }[name]
    shape = (2, int(oshape[0] * max(sc, 0.5)) + 6, int(oshape[1] * max(sc, 0.5)) + 3)
    plan = A.plan_affine(shape, np.dtype(dtype), ((sc, 0.0, ox), (0.0, sc, oy)), (2,) + oshape,
                         (1,) + tile, 1, agg, False, cval)
    assert plan.post_agg is None and plan.run_weights == (name == "k3w")
    return plan, shape


@pytest.mark.parametrize("name,dtype", [
    ("plain", "float32"), ("plain", "uint8"), ("plain", "float64"),
    ("k3i", "float32"), ("k3w", "float32"), ("k3w", "float64"),
    ("generic", "float32"), ("generic", "uint8"), ("generic", "float64"),
    ("bicubic", "float32"), ("bicubic", "uint8"), ("bicubic", "float64")])
def test_affine_strided(name, dtype):
    """Plain order 1 (150 x 200 in 64 x 48 chunks), K3i mean 4 x 4 at width
    300, K3w at offset (0.5, 0.25), the generic coarsen at 2.5, and K2q on
    its product path and with 24-row tiles."""
    from xcube_resampling_amd import _native, kernels

    plan, shape = _affine_plan(name, dtype)
    data = _payload(dtype, shape, 1)
    want = check(lambda s, o: kernels.affine(s, plan, out=o), data, f"{name} {dtype}")
    assert tuple(want.shape) == (2, plan.out_h, plan.out_w)
    if name == "bicubic":
        with _native.testing_knob("affine_bicubic_tile_h", 24):
            again = check(lambda s, o: kernels.affine(s, plan, out=o), data, f"tile_h 24 {dtype}")
        assert_bitwise_equal(again.cpu().numpy(), want.cpu().numpy(), "tile_h 24")


# ------------------------------------------------------------------ K7 -------
@pytest.mark.parametrize("agg", ["mean", "median", "mode"])
def test_coarsen_strided(agg):
    """2 x 24 x 40 float32 in 3 x 4 windows over unaligned chunks; `mode` with
    the chunk ids of categorical floats."""
    import xcube_resampling_amd.affine as A
    from xcube_resampling_amd import kernels

    shape, dy, dx = (2, 24, 40), 3, 4
    rng = np.random.default_rng(2)
    data = rng.integers(-3, 4, shape).astype(np.float32) if agg == "mode" else \
        _payload("float32", shape, 2)
    ids = A.coarsen_chunk_ids(shape, (1, 7, 12), (1, dy, dx))
    out_dtype = A._agg_dtype(agg, np.float32)
    want = check(lambda s, o: kernels.coarsen(s, dy, dx, agg, out_dtype, chunk_ids=ids, out=o),
                 data, agg)
    assert tuple(want.shape) == (2, 8, 10)


# ------------------------------------------------------------- K6 / K5 -------
@pytest.mark.parametrize("interp", ["nearest", "bilinear", "triangular"])
def test_rectify_var_strided(interp):
    """K6 at test_dtypes_gpu's synthetic positions; its `out=` keeps dense
    rows (the wrapper requires them) in a tensor with spare slices and rows."""
    import torch

    from test_dtypes_gpu import K6_SRC, k6_positions
    from xcube_resampling_amd import kernels

    ij = torch.from_numpy(k6_positions()).cuda()
    data = _payload("float32", (2,) + K6_SRC, 3)
    check(lambda s, o: kernels.rectify_var(ij, s, interp, float("nan"), out=o), data, interp,
          out_rows_dense=True)


@pytest.mark.parametrize("interp", ["nearest", "bilinear", "triangular"])
def test_rectify_fused_strided(interp):
    from test_dtypes_gpu import fused_swath
    from xcube_resampling_amd import kernels
    from xcube_resampling_amd import rectify as R

    sgm, tgm, xy, (h, w) = fused_swath()
    data = _payload("float32", (2, h, w), 4)

    def call(s, o):
        return kernels.rectify_ij_var(xy[0], xy[1], R._device_tiles(sgm, tgm, xy), tgm.height,
                                      tgm.width, tgm.x_res, -tgm.y_res, 1e-3, s, interp,
                                      float("nan"), keep_ij=False)[1]

    want = check(call, data, f"fused {interp}", has_out=False)
    assert np.isfinite(want.cpu().numpy()).mean() > 0.3


# ------------------------------------------------------------ rejections -----
def test_wrappers_reject_a_strided_innermost_dimension():
    import torch

    import xcube_resampling_amd.affine as A
    from test_dtypes_gpu import K1_H, K1_W, _k1_plans
    from xcube_resampling_amd import kernels

    def every_other(shape):
        return torch.zeros(shape[:2] + (2 * shape[2],), dtype=torch.float32,
                           device="cuda")[:, :, ::2]

    with pytest.raises(ValueError, match="innermost"):
        kernels.reproject(every_other((1, K1_H, K1_W)), _k1_plans()["gen"], "nearest", np.nan)
    plan = A.plan_affine((1, 40, 50), np.dtype(np.float32), ((0.5, 0.0, 0.0), (0.0, 0.5, 0.0)),
                         (1, 60, 80), (1, 32, 32), 1, "first", False, np.nan)
    with pytest.raises(ValueError, match="innermost"):
        kernels.affine(every_other((1, 40, 50)), plan)
    with pytest.raises(ValueError, match="innermost"):
        kernels.coarsen(every_other((1, 24, 40)), 2, 2, "mean", np.float32)
    out = every_other((1, 12, 20))
    src = torch.zeros((1, 24, 40), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="innermost"):
        kernels.coarsen(src, 2, 2, "mean", np.float32, out=out)
