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
template <> struct ScipyOut<float> {
  __device__ static inline float cast(double t) { return (float)t; }
};
template <> struct ScipyOut<double> {
  __device__ static inline double cast(double t) { return t; }
};

}  // namespace xrs
