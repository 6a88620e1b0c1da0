// xrs_rectify_bicubic.hip — K6q: bicubic (Keys a = -0.5) sampling of a variable
// at rectify's irregular source positions for gfx950; the semantics are in
// include/xrs.h (xrs_rectify_var, XRS_INTERP_BICUBIC).
//
// Rectify positions are irregular but locally smooth: a small block of target
// pixels maps to a compact, possibly rotated, patch of the swath, and the 16
// taps of neighbouring pixels overlap almost entirely.  A block of 256 threads
// owns one tile of kTileW x kTileH target pixels (32 x 16: kPx = 2 pixels per
// thread, rows ty and ty + 8) and all n slices of it:
//   1. classify: every thread reads its positions once and keeps i0, j0 and
//      the eight weights of each pixel in registers across the slices (NaN ->
//      fill, outside the source -> fill + XRS_EFLAG_STATE, as K6).
//   2. rectangle: wave reductions, then four words per wave in LDS, give the
//      min / max of i0 and of j0 over the tile's valid pixels; the tile reads
//      [imin - 1, imax + 2] x [jmin - 1, jmax + 2] in unclamped index space.  A
//      tile without a valid pixel stores fill and is done.
//   3. per slice, if the rectangle fits the launch's dynamic LDS (a block-
//      uniform decision): it is staged in the source dtype, threads walking
//      rectangle rows with consecutive columns (four loads in flight each),
//      every element from the clamped global index, so LDS holds the edge-
//      replicated values; after a barrier each pixel reads its 4 x 4 taps at
//      (j0 - jmin + a, i0 - imin + b), filters rows then the column in
//      float64, casts and stores; a barrier precedes the next slice's staging.
//      Rows are padded to an odd pitch: the lanes of a wave sit on two target
//      rows whose taps start about one staged row apart.
//   4. otherwise (scattered positions, a target far coarser than the swath)
//      the pixel's 16 taps come from global memory with clamped indices: same
//      arithmetic, same bytes out.
// One buffer, not two: a slice's staging is short against its 16-tap filter
// and a second buffer would halve the rectangles that fit.
//
// This file is compiled without packed-fp32 instructions (Makefile); all
// arithmetic is float64 without contraction in a pinned order, so matrix
// instructions have no place in it.

#include <cmath>

#include "xrs_affine.hpp"
#include "xrs_rectify.hpp"

#ifndef XRS_K6Q_PX
#define XRS_K6Q_PX 2   // target pixels per thread (timing arms: 1, 4; DESIGN.md "K6q")
#endif

namespace xrs {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTileW = 32;                       // target columns per tile
constexpr int kPassRows = kThreads / kTileW;     // target rows the block covers per pixel slot
constexpr int kPx = XRS_K6Q_PX;
constexpr int kTileH = kPassRows * kPx;          // target rows per tile
// dynamic LDS of a block: the registers (120-138 VGPRs) allow 4 blocks per CU,
// which 32 KiB each keeps resident within the CU's 160 KB; it holds a 90 x 90
// float32 or a 64 x 63 float64 rectangle, many times what a tile of a swath
// rectified near its own resolution reads
constexpr int64_t kLdsBudget = 32 * 1024;
constexpr int64_t kLdsMax = 48 * 1024;           // upper limit of the testing knob

struct BicubicArgs {
  const double* ij;
  int64_t ij_sn, dst_h, dst_w;
  const void* src;
  int64_t n, src_h, src_w, src_sn, src_sy;
  void* dst;
  int64_t dst_sn;
  double fill;
  int32_t* err_flags;
  int64_t lds_bytes;   // the staging capacity (0: every tile reads its taps from global memory)
};

enum : int { kSkip = 0, kFill = 1, kValid = 2 };   // outside the target / fill / sampled

struct Pixel {
  int32_t i0, j0;
  int state;
  CubicW wx, wy;
};

__device__ inline int32_t wave_min(int32_t v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v = min(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ inline int32_t wave_max(int32_t v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ inline int32_t wave_uniform(int32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// rows then the column, taps converted to float64 first (include/xrs.h)
template <typename T>
__device__ inline double filter16(const T (&v)[4][4], const CubicW& wx, const CubicW& wy) {
  double hr[4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
    hr[a] = cubic_sum(wx, Conv<T>::to_f64(v[a][0]), Conv<T>::to_f64(v[a][1]),
                      Conv<T>::to_f64(v[a][2]), Conv<T>::to_f64(v[a][3]));
  return cubic_sum(wy, hr[0], hr[1], hr[2], hr[3]);
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
rectify_bicubic_kernel(BicubicArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  T* stage = reinterpret_cast<T*>(smem);
  __shared__ int32_t s_red[4][kWaves];   // per wave: min i0, min j0, max i0, max j0
  const int t = threadIdx.x, tx = t % kTileW, ty = t / kTileW;
  const int wave = wave_uniform(t >> 6);
  const int32_t h = (int32_t)a.src_h, w = (int32_t)a.src_w;
  const T tfill = Conv<T>::from_f64(a.fill);
  const int64_t ntx = (a.dst_w + kTileW - 1) / kTileW, nty = (a.dst_h + kTileH - 1) / kTileH;
  const int64_t ntiles = ntx * nty;
  bool bad = false;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t tj = tile / ntx, ti = tile - tj * ntx;
    const int64_t c = ti * kTileW + tx, r0t = tj * kTileH + ty;
    // ---- 1: classify (K6's tests and truncations) ------------------------------
    Pixel px[kPx];
    int32_t imin = INT32_MAX, jmin = INT32_MAX, imax = -1, jmax = -1;
#pragma unroll
    for (int k = 0; k < kPx; ++k) {
      const int64_t r = r0t + k * kPassRows;
      Pixel& p = px[k];
      p.i0 = p.j0 = 0;
      p.state = kSkip;
      double u = 0.0, v = 0.0;
      if (r < a.dst_h && c < a.dst_w) {
        const int64_t o = r * a.dst_w + c;
        const double fi = a.ij[o], fj = a.ij[a.ij_sn + o];
        p.state = kFill;
        if (fi == fi && fj == fj) {
          if (fi >= 0.0 && fi < (double)a.src_w && fj >= 0.0 && fj < (double)a.src_h) {
            p.state = kValid;
            p.i0 = (int32_t)fi;
            p.j0 = (int32_t)fj;
            u = fi - (double)p.i0;
            v = fj - (double)p.j0;
            imin = min(imin, p.i0); imax = max(imax, p.i0);
            jmin = min(jmin, p.j0); jmax = max(jmax, p.j0);
          } else {
            bad = true;
          }
        }
      }
      p.wx = cubic_weights(u);
      p.wy = cubic_weights(v);
    }
    // ---- 2: the tile's source rectangle ---------------------------------------------
    imin = wave_min(imin); jmin = wave_min(jmin);
    imax = wave_max(imax); jmax = wave_max(jmax);
    if ((t & 63) == 0) {
      s_red[0][wave] = imin; s_red[1][wave] = jmin;
      s_red[2][wave] = imax; s_red[3][wave] = jmax;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kWaves; ++q) {
      imin = min(imin, s_red[0][q]); jmin = min(jmin, s_red[1][q]);
      imax = max(imax, s_red[2][q]); jmax = max(jmax, s_red[3][q]);
    }
    imin = wave_uniform(imin); jmin = wave_uniform(jmin);
    imax = wave_uniform(imax); jmax = wave_uniform(jmax);
    T* __restrict__ dst = static_cast<T*>(a.dst) + r0t * a.dst_w + c;
    if (imax < 0) {   // no valid pixel (block-uniform)
      for (int64_t s = 0; s < a.n; ++s) {
#pragma unroll
        for (int k = 0; k < kPx; ++k)
          if (px[k].state != kSkip)
            __builtin_nontemporal_store(tfill, dst + s * a.dst_sn + (int64_t)k * kPassRows * a.dst_w);
      }
    } else {
      const int64_t rw = (int64_t)imax - imin + 4, rh = (int64_t)jmax - jmin + 4;
      const int64_t pitch64 = rw | 1;
      const bool staged = pitch64 * rh * (int64_t)sizeof(T) <= a.lds_bytes;   // block-uniform
      const int pitch = (int)pitch64;   // (used when staged: then all of these fit an int)
      const int total = staged ? (int)(rw * rh) : 0;
      const int32_t rc0 = imin - 1, rr0 = jmin - 1;
      for (int64_t s = 0; s < a.n; ++s) {
        const T* __restrict__ src = static_cast<const T*>(a.src) + s * a.src_sn;
        if (staged) {
          // ---- 3a: stage the clamped rectangle --------------------------------------
          for (int base = t; base < total; base += 4 * kThreads) {
            T v[4];
            int o[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {   // (past the end: the last cell again, not stored)
              const int idx = min(base + q * kThreads, total - 1);
              const int i = (int)((uint32_t)idx / (uint32_t)rw), j = idx - i * (int)rw;
              const int32_t gr = min(max(rr0 + i, 0), h - 1), gc = min(max(rc0 + j, 0), w - 1);
              v[q] = src[(int64_t)gr * a.src_sy + gc];
              o[q] = i * pitch + j;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
              if (base + q * kThreads < total) stage[o[q]] = v[q];
          }
          __syncthreads();
        }
        // ---- 3b / 4: the 16 taps, filter, cast, store -------------------------------
#pragma unroll
        for (int k = 0; k < kPx; ++k) {
          const Pixel& p = px[k];
          if (p.state == kSkip) continue;
          T o = tfill;
          if (p.state == kValid) {
            T v[4][4];
            if (staged) {   // rows j0 - jmin + a <= rh - 1, columns i0 - imin + b <= rw - 1
              const T* sp = stage + (p.j0 - jmin) * pitch + (p.i0 - imin);
#pragma unroll
              for (int aa = 0; aa < 4; ++aa)
#pragma unroll
                for (int b = 0; b < 4; ++b) v[aa][b] = sp[aa * pitch + b];
            } else {
              int32_t col[4];
#pragma unroll
              for (int b = 0; b < 4; ++b) col[b] = min(max(p.i0 - 1 + b, 0), w - 1);
#pragma unroll
              for (int aa = 0; aa < 4; ++aa) {
                const T* row = src + (int64_t)min(max(p.j0 - 1 + aa, 0), h - 1) * a.src_sy;
#pragma unroll
                for (int b = 0; b < 4; ++b) v[aa][b] = row[col[b]];
              }
            }
            o = ScipyOut<T>::cast(filter16<T>(v, p.wx, p.wy));
          }
          __builtin_nontemporal_store(o, dst + s * a.dst_sn + (int64_t)k * kPassRows * a.dst_w);
        }
        if (staged) __syncthreads();   // the next slice (or tile) overwrites the rectangle
      }
    }
    __syncthreads();   // the next tile overwrites s_red
  }
  if (bad) atomicOr(a.err_flags, XRS_EFLAG_STATE);
}

}  // namespace

int rectify_bicubic_launch(const double* ij, int64_t ij_sn, int64_t dst_h, int64_t dst_w,
                           const void* src, int src_dtype, int64_t n, int64_t src_h,
                           int64_t src_w, int64_t src_sn, int64_t src_sy, void* dst,
                           int64_t dst_sn, double fill, int32_t* err_flags, hipStream_t stream) {
  // tests and timing (xrs_testing_set): every tile on the 16-tap global path;
  // the staging capacity in bytes
  const bool direct = xrs_testing_value(XRS_TESTING_RECTIFY_BICUBIC_DIRECT) == 1;
  const int64_t knob = xrs_testing_value(XRS_TESTING_RECTIFY_BICUBIC_LDS);
  const int64_t lds = direct ? 0 : (knob > 0 ? (knob < kLdsMax ? knob : kLdsMax) : kLdsBudget);
  const BicubicArgs a{ij, ij_sn, dst_h, dst_w, src, n, src_h, src_w, src_sn, src_sy,
                      dst, dst_sn, fill, err_flags, lds};
  const int64_t ntiles = ((dst_w + kTileW - 1) / kTileW) * ((dst_h + kTileH - 1) / kTileH);
  const int rc = dispatch_dtype(src_dtype, [&](auto tag) -> int {
    using T = decltype(tag);
    hipLaunchKernelGGL((rectify_bicubic_kernel<T>), dim3(grid_blocks(ntiles, 1, 1 << 22)),
                       dim3(kThreads), (size_t)lds, stream, a);
    XRS_HIP_CHECK(hipGetLastError());
    return XRS_OK;
  });
  if (rc == XRS_ERR_ARG) xrs_set_error("xrs_rectify_var: unsupported dtype");
  return rc;
}

}  // namespace xrs
