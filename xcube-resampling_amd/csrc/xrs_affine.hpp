// xrs_affine.hpp — what xrs_affine.hip (K2 / K3) and xrs_affine_bicubic.hip
// (K2q) share: the dask-image chunk tables of one axis, the chunk-local
// coordinate of an output index and scipy's output casts.
#pragma once

#include <limits>

#include "xrs_common.hpp"

namespace xrs {

struct AxisChunks {
  int64_t n;             // intermediate length along the axis
  int64_t chunk;         // dask-image output chunk size (uniform, last may be short)
  const int64_t* rel;    // per chunk: first index of the input slice
  const int64_t* len;    // per chunk: input slice length
  const double* off;     // per chunk: re-based offset (offset + M*chunk_off - rel)
  double scale;
};

// o / chunk: a 32-bit division while both fit (the usual case; a 64-bit
// division is a long software sequence on the critical path of K2)
__device__ inline int64_t chunk_of(int64_t o, int64_t chunk) {
  if (((uint64_t)o | (uint64_t)chunk) <= 0x7FFFFFFFull) return (int64_t)((uint32_t)o / (uint32_t)chunk);
  return o / chunk;
}

// chunk-local coordinate of index o: the re-based offset of its dask-image
// output chunk k plus the local index times the scale
__device__ inline double axis_coord(const AxisChunks& a, int64_t o, int64_t& k) {
  k = chunk_of(o, a.chunk);
  const int64_t ol = o - k * a.chunk;
  return a.off[k] + (double)ol * a.scale;
}

// ---- scipy output casts ----------------------------------------------------
template <typename T> struct ScipyOut {
  // integer outputs: round half away from zero, clamp to the type range
  __device__ static inline T cast(double t) {
    t = t > 0 ? t + 0.5 : t - 0.5;
    const double lo = (double)std::numeric_limits<T>::min();
    const double hi = (double)std::numeric_limits<T>::max();
    t = t > hi ? hi : t;
    t = t < lo ? lo : t;
    return (T)t;
  }
};
// int64: the clamp's upper bound (double)INT64_MAX is 2^63, one past the type,
// and scipy's C cast of it on x86 is the integer indefinite INT64_MIN (so is
// every value that rounds to 2^63 on its way through float64)
template <> struct ScipyOut<int64_t> {
  __device__ static inline int64_t cast(double t) {
    t = t > 0 ? t + 0.5 : t - 0.5;
    t = t > 9223372036854775808.0 ? 9223372036854775808.0 : t;
    t = t < -9223372036854775808.0 ? -9223372036854775808.0 : t;
    return f64_to_i64_x86(t);
  }
};
template <> struct ScipyOut<float> {
  __device__ static inline float cast(double t) { return (float)t; }
};
template <> struct ScipyOut<double> {
  __device__ static inline double cast(double t) { return t; }
};

// scipy's result for a tap of weight one whose other taps add exact zeros
// (order 0; order 1 at an integral position): t = 0.0 + v, so the value itself
// with -0 -> +0.  int64 is the one type float64 does not hold exactly: its
// values pass through float64 and the output cast as in scipy (low bits above
// 2^53 are lost, values that round to 2^63 come out as INT64_MIN).
template <typename T> __device__ inline T scipy_unit_tap(T a) { return a == (T)0 ? (T)0 : a; }
template <> __device__ inline int64_t scipy_unit_tap<int64_t>(int64_t a) {
  return ScipyOut<int64_t>::cast((double)a);
}

}  // namespace xrs
