"""The references of test_dtypes_gpu pin themselves (no GPU): the `wide`
generator, scipy's output cast at the limits of every integer type, and
numpy's float64 -> integer cast of out-of-range values, which the triangular
oracle relies on and which is the host's, not the language's."""

from __future__ import annotations

import warnings

import numpy as np
import pytest
from scipy import ndimage as ndi

from helpers import assert_bitwise_equal
from test_affine_bicubic_gpu import _cast
from test_dtypes_gpu import (INT_DTYPES, NEED, _rng, extremes, k1_oracle, k1_triangular_prestore,
                             outside, wide, K1_H, K1_W)

ALL_INTS = ["uint8", "int8", "uint16", "int16", "uint32", "int32", "int64"]

# numpy's float64 -> uint32 cast of values of 2^32 and more is not one
# function of the value: on x86 its SIMD loop gives 0 (0x80000000 for values
# below -2^31) where the scalar loop that finishes the array (and every
# boolean-mask assignment shorter than a vector) keeps the low 32 bits of the
# 64-bit conversion, the rule of xrs_common.hpp.  The same value comes out
# differently by its position in the array, so no wide case of test_dtypes_gpu
# stores such a value to uint32 (triangular reprojection and `var` leave
# uint32 out for it; uint32 differences never wrap below zero).
UINT32_ABOVE_RANGE = 2.0 ** 32


@pytest.mark.parametrize("dtype", ALL_INTS)
def test_wide_plants_the_extremes(dtype):
    info = np.iinfo(dtype)
    for shape in [(2, 24, 40), (50, 64), (3, 5)]:
        a = wide(_rng("cpu", dtype, shape), dtype, shape)
        assert a.dtype == np.dtype(dtype) and a.shape == shape
        for v in extremes(dtype):
            assert (a == v).any(), f"{dtype} {shape}: {v} missing"
    a = wide(_rng("cpu", dtype), dtype, (2, 80, 96)).astype(object)
    jump = np.abs(a[:, :, 1:] - a[:, :, :-1]) > (info.max - info.min) // 2
    assert jump.mean() > 0.15, "neighbours must regularly differ by more than half the range"
    assert ((a != info.min) & (a != info.max)).mean() > 0.7   # still mostly uniform draws


def x86_cast(x: float, dtype) -> int:
    """numpy's float64 -> integer cast on x86 as xrs_common.hpp states it, in
    Python integers: the truncating conversion to int32 (to int64 for uint32
    and int64), NaN and everything outside that type giving its minimum, then
    the low bits of the target width."""
    dt = np.dtype(dtype)
    bits = 8 * dt.itemsize
    lim = 2**63 if dt in (np.dtype(np.uint32), np.dtype(np.int64)) else 2**31
    v = int(x) if x == x and -lim <= x < lim else -lim
    v &= (1 << bits) - 1
    return v - (1 << bits) if dt.kind == "i" and v >= 1 << (bits - 1) else v


def test_x86_cast_rule_examples():
    assert x86_cast(3e9, "int32") == -2**31 and x86_cast(3e9, "uint32") == 3000000000
    assert x86_cast(-5.0, "uint8") == 251 and x86_cast(300.7, "uint8") == 44
    assert x86_cast(-1e20, "int16") == 0 and x86_cast(-1e20, "int64") == -2**63
    assert x86_cast(2.0**63, "int64") == -2**63 and x86_cast(-5.0, "uint32") == 2**32 - 5
    assert x86_cast(float("nan"), "int32") == -2**31 and x86_cast(-1.9, "int8") == -1


@pytest.mark.parametrize("dtype", ALL_INTS)
@pytest.mark.parametrize("order", [0, 1])
def test_scipy_output_cast_at_the_limits(dtype, order):
    """ndimage.affine_transform at identity == `_cast` of the float64 image:
    every type keeps its limits except int64, whose maximum (and every value
    that rounds to 2^63 as float64) comes out as INT64_MIN, and whose values
    beyond 2^53 lose their low bits (odd ones from 2^52 on already, in the
    cast's t + 0.5) — identity is not a copy."""
    info = np.iinfo(dtype)
    vals = extremes(dtype) + [info.min + 2, info.max - 2, 17, 200 if info.max > 200 else 100]
    if dtype == "int64":
        vals += [info.max - 511, info.max - 513, info.min + 513, 2**53 - 1, 2**53 + 3, 2**52 - 1]
    img = np.array(vals * 3, np.dtype(dtype)).reshape(3, -1)
    got = ndi.affine_transform(img, [1.0, 1.0], order=order, mode="constant", cval=0.0,
                               prefilter=False)
    assert_bitwise_equal(got, _cast(img.astype(np.float64), np.dtype(dtype)), f"{dtype} {order}")
    if dtype == "int64":
        flat = dict(zip(vals, got[0].tolist()))
        assert flat[info.max] == flat[info.max - 1] == flat[info.max - 511] == info.min
        assert flat[info.max - 513] == 2**63 - 1024 and flat[info.min] == info.min
        assert flat[2**53 + 1] == 2**53 and flat[2**62 + 3] == 2**62
        assert flat[-(2**53 + 1)] == -(2**53) and flat[2**52 - 1] == 2**52 - 1
        assert flat[2**53 - 1] == 2**53   # t + 0.5 is a tie from 2^52 on: odd values round to even
    else:
        assert_bitwise_equal(got, img, f"{dtype}: identity is a copy")


def test_cast_saturates_fractions():
    for dtype in ALL_INTS:
        info = np.iinfo(dtype)
        t = np.array([float(info.max) * 1.5 + 10, float(info.min) * 1.5 - 10, 2.5, -2.5, 2.4999])
        hi = info.min if dtype == "int64" else info.max
        lo = info.min
        exp = [hi, lo, 3, max(-3, info.min), 2]
        assert _cast(t, np.dtype(dtype)).tolist() == exp, dtype


@pytest.mark.parametrize("dtype", INT_DTYPES)
def test_vectorised_cast_is_the_scalar_rule(dtype):
    """The triangular oracle assigns float64 values far outside the type into
    a source-dtype array.  Its result is the kernels' bar only if that
    vectorised cast is the element-by-element rule of xrs_common.hpp: checked
    here on the very values the wide K1 case stores (restated branch ==
    oracle first).  uint32 is checked below 2^32 only (UINT32_ABOVE_RANGE)."""
    dt = np.dtype(dtype)
    data = wide(_rng("k1", dtype, "wide"), dt, (2, K1_H, K1_W))
    pre = k1_triangular_prestore(data)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        vec = pre.astype(dt)
        if dtype != "uint32":
            assert_bitwise_equal(vec, k1_oracle(data, "triangular"), "restated branch == oracle")
        keep = np.ones(pre.shape, bool)
        if dtype == "uint32":
            keep = pre < UINT32_ABOVE_RANGE
            assert keep.sum() >= NEED and (pre >= 0).all()
        else:
            assert outside(pre, dt).sum() >= NEED
    assert vec[keep].tolist() == [x86_cast(x, dt) for x in pre[keep].tolist()]
