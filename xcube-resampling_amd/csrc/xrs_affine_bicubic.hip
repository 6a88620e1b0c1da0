// xrs_affine_bicubic.hip — K2q: bicubic (Keys a = -0.5) same-CRS affine
// resampling for gfx950; the semantics are in include/xrs.h (xrs_affine_bicubic).
//
// The transform is diagonal: the source position of an output pixel depends
// on its row index for y and on its column index for x only, and an output
// tile reads one compact source rectangle.  affine_bicubic_tile_kernel works
// on one 64-column x tile_h-row output tile of one slice at a time:
//   1. entries: every thread evaluates the entry (floor index f, fraction d)
//      of its column inline from rel / len / off and keeps the four x weights
//      in registers; the first wave also evaluates the tile's row entries and
//      leaves f and the four y weights of each row in a small LDS table.  Wave
//      reductions give the min / max f of the valid columns and rows: the
//      rectangle is [fmin - 1, fmax + 2] per axis (a tile may straddle
//      dask-image chunks; nothing assumes one offset per tile).
//   2. stage: the rectangle goes to LDS in the source dtype with coalesced
//      reads, four elements in flight per thread; the edge clamp is applied
//      here, so cell (i, j) holds src[clamp(r0 + i)][clamp(c0 + j)].
//   3. horizontal: for every staged row i and tile column, h(i, column) in
//      float64 into a second LDS array (wave w takes rows w, w + 4, ...).
//   4. vertical: per output row four h rows are combined with the row's y
//      weights, cast, replaced by cval where either axis is outside, and
//      stored (non-temporal, 64 consecutive columns per wave).
// A thread owns the same column in passes 3 and 4, so both LDS arrays are
// read and written with lanes on consecutive cells: no padding is needed.
//
// The LDS a launch needs follows from the scales (span_cap); the launcher
// halves the tile height (64, 32, 16) until it fits the budget, and a launch
// whose tiles still would not fit (a scale well above 1) runs
// affine_bicubic_direct_kernel, one pixel per thread with its 16 taps read
// from global memory.  A tile whose rectangle exceeds what the launch
// allocated (not expected; it guards the LDS bounds) takes the same 16-tap
// path inside the tile kernel.
//
// This file is compiled without packed-fp32 instructions (Makefile); all
// arithmetic here is float64 without contraction, in a pinned order, so
// matrix instructions have no place in it.

#include <cmath>

#include "xrs_affine.hpp"
#include "xrs_common.hpp"

namespace xrs {
namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 64;                   // output columns per tile (one per lane)
constexpr int kWaves = kThreads / kTileW;
constexpr int kTileHMax = 64;                // output rows per tile: at most one per lane of wave 0
constexpr int kTileH = 64;                   // measured: DESIGN.md "K2q"
constexpr int kTileHMin = 16;                // lowest tile the launcher falls back to
constexpr int64_t kLdsBudget = 56 * 1024;    // dynamic LDS of a block (+ 2.3 KiB static)

struct BicubicArgs {
  const void* src;
  int64_t nt, src_h, src_w, src_st, src_sy;
  void* dst;
  int64_t out_h, out_w, dst_st, dst_sy;
  double cval;
};

struct CubicEntry {
  int32_t f;   // global source index of floor(c); -1 = outside (cval)
  double d;    // c - floor(c)
};

// order 1's position and inside test of output index o.  f lies inside the
// source for consistent tables; it is clamped so that it does for any.
__device__ inline CubicEntry cubic_entry(const AxisChunks& a, int64_t o, int64_t size) {
  int64_t k;
  const double c = axis_coord(a, o, k);
  CubicEntry e{-1, 0.0};
  if (c < 0.0 || c > (double)(a.len[k] - 1)) return e;
  const double s = floor(c);
  e.f = (int32_t)min(max(a.rel[k] + (int64_t)s, (int64_t)0), size - 1);
  e.d = c - s;
  return e;
}

__device__ inline int32_t wave_uniform(int32_t v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ inline int32_t wave_min(int32_t v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v = min(v, __shfl_xor(v, m));
  return v;
}
__device__ inline int32_t wave_max(int32_t v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v = max(v, __shfl_xor(v, m));
  return v;
}

// the pixel whose floor indices are (fy, fx) from its 16 taps in global memory
// (edge replicated)
template <typename T>
__device__ inline double bicubic_taps(const T* __restrict__ src, int64_t sy, int32_t h, int32_t w,
                                      int32_t fy, const CubicW& wy, int32_t fx, const CubicW& wx) {
  int32_t col[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) col[i] = min(max(fx - 1 + i, 0), w - 1);
  T v[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const T* row = src + (int64_t)min(max(fy - 1 + j, 0), h - 1) * sy;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[j][i] = row[col[i]];
  }
  double hr[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    hr[j] = cubic_sum(wx, Conv<T>::to_f64(v[j][0]), Conv<T>::to_f64(v[j][1]),
                      Conv<T>::to_f64(v[j][2]), Conv<T>::to_f64(v[j][3]));
  return cubic_sum(wy, hr[0], hr[1], hr[2], hr[3]);
}

// ---- K2q: LDS-tiled separable bicubic ------------------------------------------
// cap_nr x cap_nc: the staged rectangle the launch's dynamic LDS holds
// (cap_nr x kTileW float64 of h, then cap_nr x cap_nc source elements).
template <typename T>
__global__ void __launch_bounds__(kThreads)
affine_bicubic_tile_kernel(BicubicArgs a, AxisChunks ay, AxisChunks ax, int tile_h, int cap_nr,
                           int cap_nc) {
  extern __shared__ __align__(16) unsigned char smem[];
  double* hbuf = reinterpret_cast<double*>(smem);
  T* stage = reinterpret_cast<T*>(smem + (size_t)cap_nr * kTileW * sizeof(double));
  __shared__ double s_wy[kTileHMax][4];   // per tile row: the y weights
  __shared__ int32_t s_fy[kTileHMax];     // and the floor index (-1 = outside)
  __shared__ int32_t s_yrange[2];         // min / max of the valid ones
  const int tx = threadIdx.x % kTileW;
  const int ty = wave_uniform(threadIdx.x / kTileW);
  const int32_t h = (int32_t)a.src_h, w = (int32_t)a.src_w;
  const T cv = ScipyOut<T>::cast(a.cval);
  const int64_t ntx = (a.out_w + kTileW - 1) / kTileW, nty = (a.out_h + tile_h - 1) / tile_h;
  const int64_t per_slice = ntx * nty, nwork = per_slice * a.nt;
  for (int64_t wk = blockIdx.x; wk < nwork; wk += gridDim.x) {
    const int64_t t = wk / per_slice, rem = wk - t * per_slice;
    const int64_t tj = rem / ntx, ti = rem - tj * ntx;
    const int64_t oj0 = tj * tile_h, oi = ti * kTileW + tx;
    const int rows = (int)min((int64_t)tile_h, a.out_h - oj0);
    // ---- 1: entries and the source rectangle --------------------------------
    CubicEntry ex{-1, 0.0};
    if (oi < a.out_w) ex = cubic_entry(ax, oi, a.src_w);
    const CubicW wx = cubic_weights(ex.d);
    // (every wave holds the tile's 64 columns: the x range needs no LDS)
    const int32_t fxmin = wave_uniform(wave_min(ex.f >= 0 ? ex.f : INT32_MAX));
    const int32_t fxmax = wave_uniform(wave_max(ex.f));
    if (ty == 0) {
      CubicEntry ey{-1, 0.0};
      if (tx < rows) ey = cubic_entry(ay, oj0 + tx, a.src_h);
      const CubicW wy = cubic_weights(ey.d);
      s_fy[tx] = ey.f;
      s_wy[tx][0] = wy.w0;
      s_wy[tx][1] = wy.w1;
      s_wy[tx][2] = wy.w2;
      s_wy[tx][3] = wy.w3;
      const int32_t mn = wave_min(ey.f >= 0 ? ey.f : INT32_MAX), mx = wave_max(ey.f);
      if (tx == 0) {
        s_yrange[0] = mn;
        s_yrange[1] = mx;
      }
    }
    __syncthreads();
    const int32_t fymin = wave_uniform(s_yrange[0]), fymax = wave_uniform(s_yrange[1]);
    const bool any = fxmax >= 0 && fymax >= 0;   // else every pixel of the tile is cval
    const int64_t nr64 = (int64_t)fymax - fymin + 4, nc64 = (int64_t)fxmax - fxmin + 4;
    const bool tiled = any && nr64 <= cap_nr && nc64 <= cap_nc;   // block-uniform
    const T* __restrict__ src = static_cast<const T*>(a.src) + t * a.src_st;
    T* __restrict__ dst = static_cast<T*>(a.dst) + t * a.dst_st + oj0 * a.dst_sy + oi;
    if (tiled) {
      const int nr = (int)nr64, nc = (int)nc64, total = nr * nc;
      const int32_t r0 = fymin - 1, c0 = fxmin - 1;
      // ---- 2: stage the clamped rectangle ------------------------------------
      for (int base = threadIdx.x; base < total; base += 4 * kThreads) {
        T v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {   // (past the end: the last cell again, not stored)
          const int idx = min(base + u * kThreads, total - 1);
          const int i = (int)((uint32_t)idx / (uint32_t)nc), j = idx - i * nc;
          const int32_t r = min(max(r0 + i, 0), h - 1), c = min(max(c0 + j, 0), w - 1);
          v[u] = src[(int64_t)r * a.src_sy + c];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (base + u * kThreads < total) stage[base + u * kThreads] = v[u];
      }
      __syncthreads();
      // ---- 3: horizontal pass --------------------------------------------------
      const int lx = ex.f >= 0 ? ex.f - fxmin : 0;   // lx + 3 <= nc - 1
      for (int i = ty; i < nr; i += kWaves) {
        const T* s = stage + i * nc + lx;
        hbuf[i * kTileW + tx] = cubic_sum(wx, Conv<T>::to_f64(s[0]), Conv<T>::to_f64(s[1]),
                                          Conv<T>::to_f64(s[2]), Conv<T>::to_f64(s[3]));
      }
      __syncthreads();
    }
    // ---- 4: vertical pass, cast, store -----------------------------------------
    for (int q = ty; q < rows; q += kWaves) {
      const int32_t fy = s_fy[q];
      const CubicW wy{s_wy[q][0], s_wy[q][1], s_wy[q][2], s_wy[q][3]};
      double r = 0.0;
      if (tiled) {
        const double* hc = hbuf + (fy >= 0 ? fy - fymin : 0) * kTileW + tx;   // rows ly .. ly + 3 < nr
        r = cubic_sum(wy, hc[0], hc[kTileW], hc[2 * kTileW], hc[3 * kTileW]);
      } else if (any) {
        r = bicubic_taps<T>(src, a.src_sy, h, w, max(fy, 0), wy, max(ex.f, 0), wx);
      }
      const T o = (fy >= 0 && ex.f >= 0) ? ScipyOut<T>::cast(r) : cv;
      if (oi < a.out_w) __builtin_nontemporal_store(o, dst + q * a.dst_sy);
    }
    __syncthreads();   // the next tile overwrites the tables and both arrays
  }
}

// ---- per-pixel 16-tap kernel ------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(kThreads)
affine_bicubic_direct_kernel(BicubicArgs a, AxisChunks ay, AxisChunks ax) {
  const int tx = threadIdx.x % kTileW;
  const int ty = wave_uniform(threadIdx.x / kTileW);
  const T cv = ScipyOut<T>::cast(a.cval);
  const int64_t ntx = (a.out_w + kTileW - 1) / kTileW, nty = (a.out_h + kWaves - 1) / kWaves;
  const int64_t per_slice = ntx * nty, nwork = per_slice * a.nt;
  for (int64_t wk = blockIdx.x; wk < nwork; wk += gridDim.x) {
    const int64_t t = wk / per_slice, rem = wk - t * per_slice;
    const int64_t tj = rem / ntx, ti = rem - tj * ntx;
    const int64_t oj = tj * kWaves + ty, oi = ti * kTileW + tx;
    if (oj >= a.out_h || oi >= a.out_w) continue;
    const CubicEntry ey = cubic_entry(ay, oj, a.src_h), ex = cubic_entry(ax, oi, a.src_w);
    const double r = bicubic_taps<T>(static_cast<const T*>(a.src) + t * a.src_st, a.src_sy,
                                     (int32_t)a.src_h, (int32_t)a.src_w, max(ey.f, 0),
                                     cubic_weights(ey.d), max(ex.f, 0), cubic_weights(ex.d));
    const T o = (ey.f >= 0 && ex.f >= 0) ? ScipyOut<T>::cast(r) : cv;
    __builtin_nontemporal_store(o, static_cast<T*>(a.dst) + t * a.dst_st + oj * a.dst_sy + oi);
  }
}

// Upper bound of fmax - fmin + 4 over n consecutive output indices: positions
// advance by `scale` per index (chunk re-basing moves them by rounding only),
// so their floors span at most floor(|scale|*(n-1)) + 1; one more for the rounding.
inline int64_t span_cap(double scale, int64_t n) {
  const double s = fabs(scale) * (double)(n - 1);
  if (!(s < 1e6)) return 1 << 20;
  return (int64_t)floor(s) + 6;
}

template <typename T>
int launch(const BicubicArgs& a, const AxisChunks& ay, const AxisChunks& ax, hipStream_t st) {
  // tests and timing (xrs_testing_set): 1 forces the per-pixel kernel, 2 gives
  // the tile kernel the smallest rectangle, so its tiles take the in-kernel
  // 16-tap path; the tile height
  const int64_t force = xrs_testing_value(XRS_TESTING_AFFINE_BICUBIC_DIRECT);
  const int64_t th_knob = xrs_testing_value(XRS_TESTING_AFFINE_BICUBIC_TILE_H);
  const bool th_set = th_knob >= 1 && th_knob <= kTileHMax;
  int64_t tile_h = th_set ? th_knob : kTileH, cap_nr, cap_nc, lds;
  for (;; tile_h /= 2) {   // a taller rectangle than the budget holds: lower tiles, down to kTileHMin
    cap_nr = span_cap(ay.scale, tile_h);
    cap_nc = span_cap(ax.scale, kTileW);
    if (force == 2) cap_nr = cap_nc = 4;
    lds = cap_nr * kTileW * (int64_t)sizeof(double) + cap_nr * cap_nc * (int64_t)sizeof(T);
    if (lds <= kLdsBudget || th_set || tile_h / 2 < kTileHMin) break;
  }
  const int64_t ntx = (a.out_w + kTileW - 1) / kTileW;
  if (force != 1 && lds <= kLdsBudget) {
    const int64_t nwork = ntx * ((a.out_h + tile_h - 1) / tile_h) * a.nt;
    hipLaunchKernelGGL((affine_bicubic_tile_kernel<T>), dim3(grid_blocks(nwork, 1, 1 << 22)),
                       dim3(kThreads), (size_t)lds, st, a, ay, ax, (int)tile_h, (int)cap_nr,
                       (int)cap_nc);
  } else {
    const int64_t nwork = ntx * ((a.out_h + kWaves - 1) / kWaves) * a.nt;
    hipLaunchKernelGGL((affine_bicubic_direct_kernel<T>), dim3(grid_blocks(nwork, 1, 1 << 22)),
                       dim3(kThreads), 0, st, a, ay, ax);
  }
  XRS_HIP_CHECK(hipGetLastError());
  return XRS_OK;
}

}  // namespace
}  // namespace xrs

extern "C" int xrs_affine_bicubic(const void* src, int src_dtype, int64_t nt, int64_t src_h,
                                  int64_t src_w, int64_t src_st, int64_t src_sy, void* dst,
                                  int dst_dtype, int64_t out_h, int64_t out_w, int64_t dst_st,
                                  int64_t dst_sy, double scale_y, double scale_x,
                                  int64_t chunk_y, const int64_t* rel_y, const int64_t* len_y,
                                  const double* off_y, int64_t chunk_x, const int64_t* rel_x,
                                  const int64_t* len_x, const double* off_x, double cval,
                                  void* stream) {
  using namespace xrs;
  // (source sizes: the tap indices f + 2 are 32-bit)
  if (!src || !dst || !rel_y || !len_y || !off_y || !rel_x || !len_x || !off_x || nt < 1 ||
      src_h < 1 || src_w < 1 || out_h < 1 || out_w < 1 || chunk_y < 1 || chunk_x < 1 ||
      src_sy < src_w || dst_sy < out_w || src_h > INT32_MAX - 4 || src_w > INT32_MAX - 4 ||
      !std::isfinite(scale_y) || !std::isfinite(scale_x)) {
    xrs_set_error("xrs_affine_bicubic: invalid argument");
    return XRS_ERR_ARG;
  }
  if (dst_dtype != src_dtype) {
    xrs_set_error("xrs_affine_bicubic: the output dtype is the source dtype");
    return XRS_ERR_ARG;
  }
  AxisChunks ay{out_h, chunk_y, rel_y, len_y, off_y, scale_y};
  AxisChunks ax{out_w, chunk_x, rel_x, len_x, off_x, scale_x};
  BicubicArgs a{src, nt, src_h, src_w, src_st, src_sy, dst, out_h, out_w, dst_st, dst_sy, cval};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = dispatch_dtype(src_dtype, [&](auto tag) -> int {
    return launch<decltype(tag)>(a, ay, ax, st);
  });
  if (rc == XRS_ERR_ARG) xrs_set_error("xrs_affine_bicubic: unsupported dtype");
  return rc;
}
