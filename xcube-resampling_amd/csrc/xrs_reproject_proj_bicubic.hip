// xrs_reproject_proj_bicubic.hip — K1pq: bicubic (Keys a = -0.5) reprojection of
// non-separable CRS pairs for gfx950 with the projection fused, per patch of
// the target, with an LDS-staged variant of the tap reads; the semantics are in
// include/xrs.h (xrs_reproject_proj, XRS_INTERP_BICUBIC).
//
// Neighbouring target pixels of a reprojection read almost the same 4 x 4
// footprints: a small patch of the target maps to a compact, slightly rotated
// rectangle of the source.  A block of 256 threads owns one patch of kPatchW x
// kPatchH target pixels (32 x 8, one pixel per thread: the projection's
// registers dominate, as in K1p) of the launch's rows and all n slices of it.
// The patch grid lies over the rows [row_begin, row_end) of the whole raster,
// not over the tiles: every pixel looks up its own tile, and the rectangle
// lives in source index space, so a patch may straddle tiles.
//   1. classify, once per patch: the pixel centre (grid_x[c], grid_y[r]) goes
//      through the pipeline (xrs_proj.hpp: the code xrs_transform and K1p run),
//      then bilinear's per-axis index math (resolve_axis_px) with the pixel's
//      tile origin and window.  Kept in registers across the slices: the floor
//      column (global) and floor row (relative to the resident band), and the
//      eight weights.  A valid pixel raises XRS_EFLAG_BAND here for any of its
//      four clamped tap rows the band does not hold.
//   2. rectangle: wave reductions, then four words per wave in LDS, give the
//      min / max of the floor column and row over the patch's valid pixels; the
//      patch reads [fxmin - 1, fxmax + 2] x [fymin - 1, fymax + 2] in unclamped
//      index space.  A patch without a valid pixel stores fill and is done.
//   3. per slice, if the rectangle fits the launch's dynamic LDS (a block-
//      uniform decision; the product launches with none, see kLdsBudget): it
//      is staged in the source dtype, threads walking rectangle rows with
//      consecutive columns (four loads in flight each),
//      every element from the clamped index (edge replicate, then silently the
//      nearest resident row: a staged row no pixel reads raises no flag);
//      after a barrier each valid pixel reads its 4 x 4 taps at (fy - fymin +
//      a, fx - fxmin + b), filters rows then the column in float64, converts
//      and stores; a barrier precedes the next slice's staging.  Rows take an
//      odd pitch.
//   4. otherwise (the product's path; with a budget: a target far coarser than
//      the source, positions scattered by a projection singularity) the 16
//      taps come from global memory with the same clamped indices: same
//      arithmetic, same bytes out.
// The pipeline is the template (its code and registers dominate); the source
// dtype is a block-uniform switch around phases 3 / 4 and the output dtype a
// uniform branch at the store, so the library holds one kernel per pipeline.
//
// This file is compiled without packed-fp32 instructions (Makefile); all
// arithmetic is float64 without contraction in a pinned order, so matrix
// instructions have no place in it.

#include "xrs_common.hpp"
#include "xrs_proj.hpp"
#include "xrs_reproject.hpp"

namespace xrs {
namespace {

using namespace k1;

constexpr int kWaves = kThreads / 64;
constexpr int kPatchW = 32;                      // target columns per patch
constexpr int kPatchH = kThreads / kPatchW;      // target rows per patch
// dynamic LDS of a block (the staging budget).  The product stages nothing:
// on the 8192^2 UTM -> LAEA problem a 32 KiB budget (every rectangle staged)
// measured 2.44 ms against 2.21 ms with every patch on the 16-tap global path
// (5.35 against 4.96 ms on the 1.5 x finer target; DESIGN.md "K1pq",
// profiles/proj_bicubic_k1pq.jsonl): the projection bounds the kernel, the
// taps of neighbouring lanes hit the same cache lines, and the staging's two
// barriers per slice cost more than the loads they save.  The staged path
// stays behind XRS_TESTING_REPROJECT_PROJ_BICUBIC_LDS for the next
// measurement (32 KiB would keep four blocks per CU within the CU's 160 KB).
constexpr int64_t kLdsBudget = 0;
constexpr int64_t kLdsMax = 48 * 1024;           // upper limit of the testing knob

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

// what a pixel keeps from phase 1 to the slices
struct Pixel {
  bool in;          // inside the launch's rows and the raster's columns
  bool valid;       // sampled (else `fill`)
  int32_t fx, fy;   // floor column (global); floor row relative to the resident band
  CubicW wx, wy;
};

// the patch's rectangle and the row clamps, block-uniform
struct Rect {
  int32_t fxmin, fymin, fxmax, fymax;
  // tap rows relative to the band: edge replicate at the source's first / last
  // row (ylo, yhi: saturated where they cannot bind), then the band's rows
  int32_t ylo, yhi, ylast, xlast;
};

__device__ inline int32_t clamp_row(int64_t l, const Rect& rc) {   // -> a resident row
  l = min(max(l, (int64_t)rc.ylo), (int64_t)rc.yhi);
  return (int32_t)min(max(l, (int64_t)0), (int64_t)rc.ylast);
}
__device__ inline int32_t clamp_col(int64_t c, const Rect& rc) {
  return (int32_t)min(max(c, (int64_t)0), (int64_t)rc.xlast);
}

// ---- phases 3 / 4 for one source dtype: every slice of the patch --------------
template <typename T>
__device__ inline void patch_slices(const GatherArgs& ga, unsigned char* smem, int64_t lds_bytes,
                                    bool out_f32, const Pixel& p, const Rect& rc, int64_t dst_off) {
  T* stage = reinterpret_cast<T*>(smem);
  const int t = threadIdx.x;
  const int64_t rw = (int64_t)rc.fxmax - rc.fxmin + 4, rh = (int64_t)rc.fymax - rc.fymin + 4;
  const int64_t pitch64 = rw | 1;
  const bool staged = pitch64 * rh * (int64_t)sizeof(T) <= lds_bytes;   // block-uniform
  const int pitch = (int)pitch64;   // (used when staged: then all of these fit an int)
  const int total = staged ? (int)(rw * rh) : 0;
  const int64_t rc0 = (int64_t)rc.fxmin - 1, rr0 = (int64_t)rc.fymin - 1;
  for (int64_t s = 0; s < ga.n; ++s) {
    const T* __restrict__ src = static_cast<const T*>(ga.src) + s * ga.src_sn;
    if (staged) {
      // ---- 3a: stage the clamped rectangle ------------------------------------------
      for (int base = t; base < total; base += 4 * kThreads) {
        T v[4];
        int o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {   // (past the end: the last cell again, not stored)
          const int idx = min(base + q * kThreads, total - 1);
          const int i = (int)((uint32_t)idx / (uint32_t)rw), j = idx - i * (int)rw;
          v[q] = src[(int64_t)clamp_row(rr0 + i, rc) * ga.src_sy + clamp_col(rc0 + j, rc)];
          o[q] = i * pitch + j;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (base + q * kThreads < total) stage[o[q]] = v[q];
      }
      __syncthreads();
    }
    // ---- 3b / 4: the 16 taps, filter, convert, store ---------------------------------
    if (p.in) {
      double out = ga.fill;
      if (p.valid) {
        T v[4][4];
        if (staged) {   // rows fy - fymin + a <= rh - 1, columns fx - fxmin + b <= rw - 1
          const T* sp = stage + (p.fy - rc.fymin) * pitch + (p.fx - rc.fxmin);
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) v[a][b] = sp[a * pitch + b];
        } else {
          int32_t col[4];
#pragma unroll
          for (int b = 0; b < 4; ++b) col[b] = clamp_col((int64_t)p.fx - 1 + b, rc);
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            const T* row = src + (int64_t)clamp_row((int64_t)p.fy - 1 + a, rc) * ga.src_sy;
#pragma unroll
            for (int b = 0; b < 4; ++b) v[a][b] = row[col[b]];
          }
        }
        // rows then the column, taps converted to float64 first (include/xrs.h)
        double hr[4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
          hr[a] = cubic_sum(p.wx, Conv<T>::to_f64(v[a][0]), Conv<T>::to_f64(v[a][1]),
                            Conv<T>::to_f64(v[a][2]), Conv<T>::to_f64(v[a][3]));
        out = cubic_sum(p.wy, hr[0], hr[1], hr[2], hr[3]);
      }
      const int64_t o = s * ga.dst_sn + dst_off;
      if (out_f32)
        __builtin_nontemporal_store((float)out, static_cast<float*>(ga.dst) + o);
      else
        __builtin_nontemporal_store(out, static_cast<double*>(ga.dst) + o);
    }
    if (staged) __syncthreads();   // the next slice (or patch) overwrites the rectangle
  }
}

template <int K0, int K1, int FAST>
__global__ void __launch_bounds__(kThreads)
gather_proj_bicubic_kernel(GatherArgs a, XrsProjStep s0, XrsProjStep s1, DivU32 div_th,
                           DivU32 div_tw, int64_t lds_bytes, int src_dtype, int out_f32) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ int32_t s_red[4][kWaves];   // per wave: min fx, min fy, max fx, max fy
  const proj::Pipeline<K0, K1, FAST> pipe(s0, s1);
  const Geometry& g = a.g;
  const int t = threadIdx.x, tx = t % kPatchW, ty = t / kPatchW;
  const int wave = wave_uniform(t >> 6);
  const int64_t npx = (g.dst_w + kPatchW - 1) / kPatchW;
  const int64_t npy = (g.row_end - g.row_begin + kPatchH - 1) / kPatchH;
  int32_t eflags = 0;
  // each XCD walks one contiguous slice of the row-major patch list: the source
  // rows a patch row fetched into that XCD's L2 serve the next patch row
  const XcdSlice sl = xcd_slice(npx * npy);
  for (int64_t patch = sl.first; patch < sl.end; patch += sl.step) {
    const int64_t pj = patch / npx, pi = patch - pj * npx;
    // rows and columns are < 2^31 (checked at launch)
    const int64_t c64 = pi * kPatchW + tx, r64 = g.row_begin + pj * kPatchH + ty;
    Pixel p;
    p.in = c64 < g.dst_w && r64 < g.row_end;
    // lanes past the raster's edge repeat its last pixel (and store nothing)
    const uint32_t c = (uint32_t)min(c64, g.dst_w - 1), r = (uint32_t)min(r64, g.row_end - 1);
    // ---- 1: classify ------------------------------------------------------------------
    double px = g.src_x[c], py = g.src_y[r];   // the target pixel centre
    pipe(s0, s1, px, py);
    // the gather's arguments re-read after the projection (kernel_arg_after:
    // kept live through it they spill, as in K1p)
    const GatherArgs ga = kernel_arg_after<GatherArgs>(px);
    const Geometry& gg = ga.g;
    const uint32_t tile = div_th.div(r) * (uint32_t)gg.ntiles_x + div_tw.div(c);
    const float x0 = gg.tile_x0[tile], y0 = gg.tile_y0[tile];
    const int64_t wi0 = gg.tile_win[2 * tile], wj0 = gg.tile_win[2 * tile + 1];
    AxisEntry ex{-1, -1, 0.0}, ey{-1, -1, 0.0};
    if (p.in) {
      ex = resolve_axis_px<XRS_INTERP_BILINEAR>(px, x0, gg.x_res, gg.win_w, wi0, gg.src_w, 0,
                                                gg.src_w, eflags);
      ey = resolve_axis_px<XRS_INTERP_BILINEAR>(py, y0, gg.neg_y_res, gg.win_h, wj0, gg.src_h,
                                                gg.src_row0, gg.src_rows, eflags);
    }
    p.valid = ex.f >= 0 && ex.c >= 0 && ey.f >= 0 && ey.c >= 0;
    p.fx = ex.f;
    p.fy = ey.f;
    p.wx = cubic_weights(ex.d);
    p.wy = cubic_weights(ey.d);
    Rect rc;
    rc.ylo = (int32_t)max(-gg.src_row0, (int64_t)-4);
    rc.yhi = (int32_t)min(max(gg.src_h - 1 - gg.src_row0, (int64_t)-4), (int64_t)INT32_MAX);
    rc.ylast = (int32_t)max(gg.src_rows - 1, (int64_t)0);
    rc.xlast = (int32_t)(gg.src_w - 1);
    if (p.valid) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {   // the four edge-replicated tap rows
        const int64_t l = min(max((int64_t)p.fy - 1 + k, (int64_t)rc.ylo), (int64_t)rc.yhi);
        if (l < 0 || l >= gg.src_rows) eflags |= XRS_EFLAG_BAND;
      }
    }
    // ---- 2: the patch's source rectangle ----------------------------------------------
    int32_t fxmin = p.valid ? p.fx : INT32_MAX, fymin = p.valid ? p.fy : INT32_MAX;
    int32_t fxmax = p.valid ? p.fx : -1, fymax = p.valid ? p.fy : -1;
    fxmin = wave_min(fxmin); fymin = wave_min(fymin);
    fxmax = wave_max(fxmax); fymax = wave_max(fymax);
    if ((t & 63) == 0) {
      s_red[0][wave] = fxmin; s_red[1][wave] = fymin;
      s_red[2][wave] = fxmax; s_red[3][wave] = fymax;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kWaves; ++q) {
      fxmin = min(fxmin, s_red[0][q]); fymin = min(fymin, s_red[1][q]);
      fxmax = max(fxmax, s_red[2][q]); fymax = max(fymax, s_red[3][q]);
    }
    rc.fxmin = wave_uniform(fxmin); rc.fymin = wave_uniform(fymin);
    rc.fxmax = wave_uniform(fxmax); rc.fymax = wave_uniform(fymax);
    const int64_t dst_off = ((int64_t)r - gg.row_begin) * ga.dst_sy + c;
    if (rc.fxmax < 0) {   // no valid pixel (block-uniform)
      if (p.in) {
        for (int64_t s = 0; s < ga.n; ++s) {
          const int64_t o = s * ga.dst_sn + dst_off;
          if (out_f32)
            __builtin_nontemporal_store((float)ga.fill, static_cast<float*>(ga.dst) + o);
          else
            __builtin_nontemporal_store(ga.fill, static_cast<double*>(ga.dst) + o);
        }
      }
    } else {
      switch (src_dtype) {   // block-uniform
#define XRS_PS(CODE, T) \
  case CODE: patch_slices<T>(ga, smem, lds_bytes, out_f32 != 0, p, rc, dst_off); break;
        XRS_PS(XRS_DTYPE_U8, uint8_t)
        XRS_PS(XRS_DTYPE_I8, int8_t)
        XRS_PS(XRS_DTYPE_U16, uint16_t)
        XRS_PS(XRS_DTYPE_I16, int16_t)
        XRS_PS(XRS_DTYPE_U32, uint32_t)
        XRS_PS(XRS_DTYPE_I32, int32_t)
        XRS_PS(XRS_DTYPE_I64, int64_t)
        XRS_PS(XRS_DTYPE_F32, float)
        XRS_PS(XRS_DTYPE_F64, double)
#undef XRS_PS
        default: break;
      }
    }
    __syncthreads();   // the next patch overwrites s_red
  }
  if (eflags) atomicOr(g.err_flags, eflags);
}

struct Launch {
  GatherArgs a;
  XrsProjStep s0, s1;
  int src_dtype, out_f32;
  int64_t lds;
  hipStream_t stream;
};

template <int K0, int K1, int FAST>
void launch_kernel(const Launch& l) {
  const Geometry& g = l.a.g;
  const int64_t npatch = ((g.dst_w + kPatchW - 1) / kPatchW) *
                         ((g.row_end - g.row_begin + kPatchH - 1) / kPatchH);
  const DivU32 dh = DivU32::make((uint32_t)g.tile_h), dw = DivU32::make((uint32_t)g.tile_w);
  hipLaunchKernelGGL((gather_proj_bicubic_kernel<K0, K1, FAST>),
                     dim3(grid_blocks(npatch, 1, 1 << 22)), dim3(kThreads), (size_t)l.lds,
                     l.stream, l.a, l.s0, l.s1, dh, dw, l.lds, l.src_dtype, l.out_f32);
}

template <int K0, int K1>
int launch_pipeline(const Launch& l) {
  // the same pipeline code as xrs_transform and K1p (proj::fast_kind picks it there too)
  if constexpr (K0 == XRS_PROJ_LAEA_INV && K1 == XRS_PROJ_TMERC_FWD) {
    const int fast = xrs_testing_value(XRS_TESTING_PROJ_TWO_STEP) ? proj::kFastNone
                                                                  : proj::fast_kind(K0, K1, l.s0);
    if (fast == proj::kFastObliq)
      launch_kernel<K0, K1, proj::kFastObliq>(l);
    else if (fast == proj::kFastEquit)
      launch_kernel<K0, K1, proj::kFastEquit>(l);
    else
      launch_kernel<K0, K1, proj::kFastNone>(l);
  } else {
    launch_kernel<K0, K1, proj::kFastNone>(l);
  }
  XRS_HIP_CHECK(hipGetLastError());
  return XRS_OK;
}

}  // namespace

int k1::launch_proj_bicubic(const GatherArgs& a, const XrsProjStep& s0, const XrsProjStep& s1,
                            int k0, int k1, int src_dtype, int dst_dtype, hipStream_t stream) {
  // tests and timing (xrs_testing_set): the staging capacity in bytes; every
  // patch on the 16-tap global path whatever the capacity
  const bool direct = xrs_testing_value(XRS_TESTING_REPROJECT_PROJ_BICUBIC_DIRECT) == 1;
  const int64_t knob = xrs_testing_value(XRS_TESTING_REPROJECT_PROJ_BICUBIC_LDS);
  const int64_t lds = direct ? 0 : (knob > 0 ? (knob < kLdsMax ? knob : kLdsMax) : kLdsBudget);
  const Launch l{a, s0, s1, src_dtype, dst_dtype == XRS_DTYPE_F32, lds, stream};
  return proj::dispatch_pipeline(k0, k1, [&](auto c0, auto c1) {
    return launch_pipeline<decltype(c0)::value, decltype(c1)::value>(l);
  });
}

}  // namespace xrs
