// xrs_rectify.hpp — what xrs_rectify.hip (K4 / K5 / K6) and
// xrs_rectify_bicubic.hip (K6q) share: the launcher xrs_rectify_var hands
// XRS_INTERP_BICUBIC to.
#pragma once

#include "xrs_common.hpp"

namespace xrs {

// K6q (xrs_rectify_bicubic.hip): xrs_rectify_var's arguments, validated by the
// caller (pointers, shapes, strides, src_h and src_w <= INT32_MAX - 4).
int rectify_bicubic_launch(const double* ij, int64_t ij_sn, int64_t dst_h, int64_t dst_w,
                           const void* src, int src_dtype, int64_t n, int64_t src_h,
                           int64_t src_w, int64_t src_sn, int64_t src_sy, void* dst,
                           int64_t dst_sn, double fill, int32_t* err_flags, hipStream_t stream);

}  // namespace xrs
