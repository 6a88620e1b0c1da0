// xrs_reproject_bicubic.hip — K1q: bicubic (Keys a = -0.5) reprojection gather
// for gfx950; the semantics are in include/xrs.h (xrs_reproject,
// XRS_INTERP_BICUBIC).
//
// Separable CRS pairs (coord_mode 0 / 2) run gather_bicubic_kernel.  The
// filter is separable and, for a separable transformation, so are the sample
// positions: the horizontally filtered value h(j, c) of source row j at target
// column c does not depend on the target row.  A work item (K1b's: one tile x
// one 512-column segment x one band of target rows, each lane two columns
// kThreads apart) therefore filters a source row ONCE and keeps the result
// for every target row that wants it:
//   * per column, in registers for the whole item: the four clamped tap byte
//     offsets and the four x weights;
//   * a ring of four h rows (float64, two per lane), keyed by the global floor
//     row f of the target row served last: slot i holds source row
//     clamp(f - 1 + i).  f comes from the row entry by readlane, so the key
//     and every decision on it are wave-uniform: the ring moves by register
//     copies under a uniform switch (no dynamic register index).  A target
//     row whose f is s = 0..3 rows further shifts the ring by s and filters s
//     new rows (s = 0: upsampling, nothing is read); anything else — the first
//     row of an item or of a dim-0 slice, a step of four or more, a step
//     backwards — refills all four.  Clamped rows repeat in the ring like any
//     other row (slot i is always clamp(f - 1 + i)).
//   * memory-level parallelism: target rows go in units of 8.  The shifts of a
//     unit are known from the row entries before any load, so the unit picks
//     its schedule: all s <= 1 -> the (at most) 8 new source rows of all 8
//     target rows are requested together; all s <= 2 -> two groups of 4 target
//     rows x 2 source rows; else four groups of 2 x 4.  Every group has up to
//     8 source rows x 4 taps x 2 columns in flight, in the same registers.
//     The stores of a group (non-temporal) are issued after the next group's
//     loads, as in K1b.
// Each source row is read once per item (plus the three ring rows an item
// shares with the band above it); no LDS.
//
// Non-separable pairs (coord_mode 1) run gather_bicubic_2d_kernel: K1c's work
// decomposition and per-pixel index math with the 16 taps of a pixel read
// directly.
//
// This file is compiled without packed-fp32 instructions (Makefile); all
// arithmetic here is float64 without contraction.

#include <type_traits>

#include "xrs_common.hpp"
#include "xrs_reproject.hpp"

namespace xrs {
namespace {

using namespace k1;

constexpr int kQUnit = 8;   // target rows per scheduling unit (and the most source rows in flight)

// K1q's work shape per output width (measured: DESIGN.md §3 "K1q, bicubic")
template <typename O>
struct K1qShape {
  static constexpr int px = 2;
  static constexpr int band = 64;
  static constexpr int segw = kThreads * px;
};

// tap k (0..3) of an axis whose floor index is the global f: f - 1 + k, edge replicated
__device__ inline int64_t cubic_tap(int64_t f, int k, int64_t size) {
  return min(max(f - 1 + k, (int64_t)0), size - 1);
}
// a global source row in the band held on this device; a row the band does
// not hold is reported and replaced by the nearest one it holds (a valid address)
__device__ inline int32_t band_row(int64_t grow, int64_t band0, int64_t band_len, int32_t& eflags) {
  const int64_t l = grow - band0;
  if (l >= 0 && l < band_len) return (int32_t)l;
  eflags |= XRS_EFLAG_BAND;
  return (int32_t)min(max(l, (int64_t)0), max(band_len - 1, (int64_t)0));
}

template <int N>
using Int = std::integral_constant<int, N>;

// ---- K1q: separable bicubic gather -------------------------------------------
template <typename T, typename O>
__global__ void __launch_bounds__(kThreads)
gather_bicubic_kernel(GatherArgs a, int64_t ty0, int64_t nsegs, int64_t bands_per_tile,
                      int64_t segs_per_tile, int64_t nwork) {
  const Geometry& g = a.g;
  constexpr int kPx = K1qShape<O>::px;
  constexpr int64_t kNoRow = INT64_MIN / 2;   // ring key: nothing held
  static_assert(64 % kQUnit == 0, "a 64-row entry chunk holds whole units");
  const O fill = Conv<O>::from_f64(a.fill);
  const int lane = (int)(threadIdx.x & 63);
  int32_t eflags = 0;
  // the XCDs take whole bands in turn (XCD x: bands x, x + 8, ...)
  const int64_t xcd = blockIdx.x & 7;
  for (int64_t i = blockIdx.x >> 3;; i += gridDim.x >> 3) {
    const int64_t m = i / nsegs;
    const int64_t w = (m * 8 + xcd) * nsegs + (i - m * nsegs);
    if (w >= nwork) break;
    WorkItem it;
    if (!work_item(g, w, ty0, nsegs, bands_per_tile, segs_per_tile, it)) continue;
    const int ncols = (int)(it.c1 - it.c0);
    const float x0 = g.tile_x0[it.t];
    const int64_t wi0 = g.tile_win[2 * it.t];
    const float y0 = g.tile_y0[it.t];
    const int64_t wj0 = g.tile_win[2 * it.t + 1];
    // ---- the item's columns (as K1b: coordinates read or generated) --------
    double sx[kPx];
    if (g.xgen) {
      const ColumnGen cg = reinterpret_cast<const ColumnGen*>(g.src_x)[it.tx];
      const double m1 = g.src_x[4 * g.ntiles_x], m2 = g.src_x[4 * g.ntiles_x + 1];
      const int last = (int)cg.n - 1, k0 = (int)(it.c0 - it.tx * g.tile_w);
#pragma unroll
      for (int k = 0; k < kPx; ++k) {
        const int kk = k0 + min((int)threadIdx.x + k * kThreads, ncols - 1);
        const double v = kk == last ? cg.stop : (double)kk * cg.step + cg.start;
        sx[k] = (v * m1) * m2;
      }
    } else {
#pragma unroll
      for (int k = 0; k < kPx; ++k) {
        const int lc = (int)threadIdx.x + k * kThreads;
        sx[k] = g.src_x[it.c0 + min(lc, ncols - 1)];
      }
    }
    const int64_t ry0 = it.r0 + lane;
    const double sy0 = g.src_y[min(ry0, it.r1 - 1)];
    // per column: is it inside the source, its four tap byte offsets in a row
    // (< 2^31: checked at launch) and its x weights
    bool xok[kPx];
    uint32_t xo[kPx][4];
    CubicW wx[kPx];
#pragma unroll
    for (int k = 0; k < kPx; ++k) {
      const int lc = (int)threadIdx.x + k * kThreads;
      AxisEntry e{-1, -1, 0.0};
      if (lc < ncols)
        e = resolve_axis<XRS_INTERP_BILINEAR>(sx[k], x0, g.x_res, g.win_w, wi0, g.src_w, 0,
                                              g.src_w, eflags);
      xok[k] = e.f >= 0 && e.c >= 0;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        xo[k][j] = (uint32_t)cubic_tap(max(e.f, 0), j, g.src_w) * (uint32_t)sizeof(T);
      wx[k] = cubic_weights(e.d);
    }
    const uint32_t row_bytes = (uint32_t)(g.src_w * (int64_t)sizeof(T));
    // ---- the item's rows: lane q holds the entry of row ybase + q ----------
    int32_t yf = -1, yc = -1;
    double yd = 0.0;
    int64_t ybase = it.r0;
    if (ry0 < it.r1) {
      const AxisEntry e = resolve_axis<XRS_INTERP_BILINEAR>(sy0, y0, g.neg_y_res, g.win_h, wj0,
                                                            g.src_h, g.src_row0, g.src_rows, eflags);
      yf = e.f;
      yc = e.c;
      yd = e.d;
    }
    for (int64_t sn = 0; sn < a.n; ++sn) {
      const T* __restrict__ src = static_cast<const T*>(a.src) + sn * a.src_sn;
      O* __restrict__ dst = static_cast<O*>(a.dst) + sn * a.dst_sn - g.row_begin * a.dst_sy + it.c0;
      double h[4][kPx];        // the ring: h[i][k] = filtered source row clamp(kf - 1 + i)
      int64_t kf = kNoRow;     // a new slice restarts the ring, not the column state
      // stores deferred by one group (issued after the next group's loads)
      O outv[kQUnit][kPx];
      int64_t rprev = 0;
      int nprev = 0;
      auto flush = [&]() {
#pragma unroll
        for (int q = 0; q < kQUnit; ++q) {
          if (q >= nprev) break;
#pragma unroll
          for (int k = 0; k < kPx; ++k) {
            const int lc = (int)threadIdx.x + k * kThreads;
            if (lc < ncols) __builtin_nontemporal_store(outv[q][k], &dst[(rprev + q) * a.dst_sy + lc]);
          }
        }
      };
      for (int64_t r = it.r0; r < it.r1; r += kQUnit) {
        if (r < ybase || r >= ybase + 64) {   // wave-uniform; once per item for bands <= 64
          ybase = r;
          const int64_t ry = r + lane;
          AxisEntry e{-1, -1, 0.0};
          if (ry < it.r1)
            e = resolve_axis<XRS_INTERP_BILINEAR>(g.src_y[ry], y0, g.neg_y_res, g.win_h, wj0,
                                                  g.src_h, g.src_row0, g.src_rows, eflags);
          yf = e.f;
          yc = e.c;
          yd = e.d;
        }
        const int j0 = (int)(r - ybase);
        // the unit's row entries and ring shifts (all wave-uniform): rows
        // outside the source (and past r1: they hold -1) leave the ring alone
        bool ok[kQUnit];
        int64_t fg[kQUnit];
        double ed[kQUnit];
        int sh[kQUnit];
        int smax = 0;
        int64_t kfu = kf;
#pragma unroll
        for (int q = 0; q < kQUnit; ++q) {
          const int32_t ef = __builtin_amdgcn_readlane(yf, j0 + q);
          const int32_t ec = __builtin_amdgcn_readlane(yc, j0 + q);
          const uint64_t db = __builtin_bit_cast(uint64_t, yd);
          const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)db, j0 + q);
          const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(db >> 32), j0 + q);
          ed[q] = __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
          ok[q] = ef >= 0 && ec >= 0;
          fg[q] = g.src_row0 + ef;
          sh[q] = 0;
          if (ok[q]) {
            const int64_t step = fg[q] - kfu;
            sh[q] = (kfu != kNoRow && step >= 0 && step <= 3) ? (int)step : 4;
            kfu = fg[q];
          }
          smax = max(smax, sh[q]);
        }
        // G target rows from row r + Q0 of the unit, each filtering up to its
        // last B ring slots anew (B >= its shift)
        auto group = [&](auto q0_, auto g_, auto b_) {
          constexpr int Q0 = decltype(q0_)::value, G = decltype(g_)::value, B = decltype(b_)::value;
          if (r + Q0 >= it.r1) return;
          T raw[G][B][4][kPx];
#pragma unroll
          for (int qq = 0; qq < G; ++qq) {
            const int q = Q0 + qq;
#pragma unroll
            for (int j = 0; j < B; ++j) {
              const int slot = 4 - B + j;
              if (slot < 4 - sh[q]) continue;
              const int32_t lrow = band_row(cubic_tap(fg[q], slot, g.src_h), g.src_row0,
                                            g.src_rows, eflags);
              const __amdgpu_buffer_rsrc_t rs = row_rsrc(src + (int64_t)lrow * a.src_sy, row_bytes);
#pragma unroll
              for (int k = 0; k < kPx; ++k)
#pragma unroll
                for (int t = 0; t < 4; ++t) raw[qq][j][t][k] = row_at<T>(rs, xo[k][t]);
            }
          }
          flush();
#pragma unroll
          for (int qq = 0; qq < G; ++qq) {
            const int q = Q0 + qq;
            if (!ok[q]) {
#pragma unroll
              for (int k = 0; k < kPx; ++k) outv[qq][k] = fill;
              continue;
            }
            switch (sh[q]) {   // the ring moves up by the shift
              case 1:
#pragma unroll
                for (int k = 0; k < kPx; ++k) { h[0][k] = h[1][k]; h[1][k] = h[2][k]; h[2][k] = h[3][k]; }
                break;
              case 2:
#pragma unroll
                for (int k = 0; k < kPx; ++k) { h[0][k] = h[2][k]; h[1][k] = h[3][k]; }
                break;
              case 3:
#pragma unroll
                for (int k = 0; k < kPx; ++k) h[0][k] = h[3][k];
                break;
              default: break;
            }
#pragma unroll
            for (int j = 0; j < B; ++j) {
              const int slot = 4 - B + j;
              if (slot < 4 - sh[q]) continue;
#pragma unroll
              for (int k = 0; k < kPx; ++k)
                h[slot][k] = cubic_sum(wx[k], Conv<T>::to_f64(raw[qq][j][0][k]),
                                       Conv<T>::to_f64(raw[qq][j][1][k]),
                                       Conv<T>::to_f64(raw[qq][j][2][k]),
                                       Conv<T>::to_f64(raw[qq][j][3][k]));
            }
            const CubicW wy = cubic_weights(ed[q]);
#pragma unroll
            for (int k = 0; k < kPx; ++k)
              outv[qq][k] = xok[k] ? Conv<O>::from_f64(cubic_sum(wy, h[0][k], h[1][k], h[2][k], h[3][k]))
                                   : fill;
          }
          rprev = r + Q0;
          nprev = (int)min((int64_t)G, it.r1 - rprev);
        };
        if (smax <= 1) {
          group(Int<0>{}, Int<8>{}, Int<1>{});
        } else if (smax <= 2) {
          group(Int<0>{}, Int<4>{}, Int<2>{});
          group(Int<4>{}, Int<4>{}, Int<2>{});
        } else {
          group(Int<0>{}, Int<2>{}, Int<4>{});
          group(Int<2>{}, Int<2>{}, Int<4>{});
          group(Int<4>{}, Int<2>{}, Int<4>{});
          group(Int<6>{}, Int<2>{}, Int<4>{});
        }
        kf = kfu;
      }
      flush();
    }
  }
  if (eflags) atomicOr(g.err_flags, eflags);
}

// ---- per-pixel bicubic gather (2-D coordinate tables) --------------------------
// K1c's decomposition and per-pixel entries; the 16 taps of kRows2D x kPx
// pixels of a slice are requested together.
template <typename T, typename O>
__global__ void __launch_bounds__(kThreads)
gather_bicubic_2d_kernel(GatherArgs a, int64_t ty0, int64_t nsegs, int64_t bands_per_tile,
                         int64_t segs_per_tile, int64_t nwork) {
  const Geometry& g = a.g;
  const O fill = Conv<O>::from_f64(a.fill);
  int32_t eflags = 0;
  for (XcdGroups sl = xcd_groups(nwork, nsegs);; sl.i += sl.step) {
    const int64_t w = sl.item();
    if (w >= nwork) break;
    WorkItem it;
    if (!work_item(g, w, ty0, nsegs, bands_per_tile, segs_per_tile, it)) continue;
    const int ncols = (int)(it.c1 - it.c0);
    const float x0 = g.tile_x0[it.t], y0 = g.tile_y0[it.t];
    const int64_t wi0 = g.tile_win[2 * it.t], wj0 = g.tile_win[2 * it.t + 1];
    for (int64_t r = it.r0; r < it.r1; r += kRows2D) {
      bool in[kRows2D][kPx], ok[kRows2D][kPx];
      int64_t ro[kRows2D][kPx][4];    // tap rows: element offsets in a slice
      int32_t co[kRows2D][kPx][4];    // tap columns
      CubicW wx[kRows2D][kPx], wy[kRows2D][kPx];
#pragma unroll
      for (int q = 0; q < kRows2D; ++q)
#pragma unroll
        for (int k = 0; k < kPx; ++k) {
          const int lc = (int)threadIdx.x + k * kThreads;
          in[q][k] = r + q < it.r1 && lc < ncols;
          const int64_t p = in[q][k] ? (r + q) * g.dst_w + it.c0 + lc : it.r0 * g.dst_w + it.c0;
          const double sx = g.src_x[p], sy = g.src_y[p];
          AxisEntry ex{-1, -1, 0.0}, ey{-1, -1, 0.0};
          if (in[q][k]) {
            ex = resolve_axis_px<XRS_INTERP_BILINEAR>(sx, x0, g.x_res, g.win_w, wi0, g.src_w, 0,
                                                      g.src_w, eflags);
            ey = resolve_axis_px<XRS_INTERP_BILINEAR>(sy, y0, g.neg_y_res, g.win_h, wj0, g.src_h,
                                                      g.src_row0, g.src_rows, eflags);
          }
          ok[q][k] = ex.f >= 0 && ex.c >= 0 && ey.f >= 0 && ey.c >= 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            // pixels that are `fill` read element 0 of the band (a valid address)
            ro[q][k][j] = ok[q][k] ? (int64_t)band_row(cubic_tap(g.src_row0 + ey.f, j, g.src_h),
                                                       g.src_row0, g.src_rows, eflags) * a.src_sy
                                   : 0;
            co[q][k][j] = ok[q][k] ? (int32_t)cubic_tap(ex.f, j, g.src_w) : 0;
          }
          wx[q][k] = cubic_weights(ex.d);
          wy[q][k] = cubic_weights(ey.d);
        }
      for (int64_t sn = 0; sn < a.n; ++sn) {
        const T* src = static_cast<const T*>(a.src) + sn * a.src_sn;
        O* dst = static_cast<O*>(a.dst) + sn * a.dst_sn + (r - g.row_begin) * a.dst_sy + it.c0;
        T t[kRows2D][kPx][4][4];
#pragma unroll
        for (int q = 0; q < kRows2D; ++q)
#pragma unroll
          for (int k = 0; k < kPx; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
              for (int i = 0; i < 4; ++i) t[q][k][j][i] = src[ro[q][k][j] + co[q][k][i]];
#pragma unroll
        for (int q = 0; q < kRows2D; ++q)
#pragma unroll
          for (int k = 0; k < kPx; ++k) {
            if (!in[q][k]) continue;
            double hr[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
              hr[j] = cubic_sum(wx[q][k], Conv<T>::to_f64(t[q][k][j][0]), Conv<T>::to_f64(t[q][k][j][1]),
                                Conv<T>::to_f64(t[q][k][j][2]), Conv<T>::to_f64(t[q][k][j][3]));
            const O out = ok[q][k] ? Conv<O>::from_f64(cubic_sum(wy[q][k], hr[0], hr[1], hr[2], hr[3]))
                                   : fill;
            dst[q * a.dst_sy + (int)threadIdx.x + k * kThreads] = out;
          }
      }
    }
  }
  if (eflags) atomicOr(g.err_flags, eflags);
}

template <typename T, typename O>
int launch(const GatherArgs& a, int coord_mode, hipStream_t stream) {
  if (coord_mode != 1) {
    const Work k = work_of(a, K1qShape<O>::band, K1qShape<O>::segw);
    hipLaunchKernelGGL((gather_bicubic_kernel<T, O>), dim3(k.nb), dim3(kThreads), 0, stream,
                       k.args, k.ty0, k.nsegs, k.bands_per_tile, k.segs_per_tile, k.nwork);
  } else {
    const Work k = work_of(a);
    hipLaunchKernelGGL((gather_bicubic_2d_kernel<T, O>), dim3(k.nb), dim3(kThreads), 0, stream,
                       k.args, k.ty0, k.nsegs, k.bands_per_tile, k.segs_per_tile, k.nwork);
  }
  XRS_HIP_CHECK(hipGetLastError());
  return XRS_OK;
}

}  // namespace

int k1::launch_bicubic(const GatherArgs& a, int src_dtype, int dst_dtype, int coord_mode,
                       hipStream_t stream) {
  return dispatch_dtype(src_dtype, [&](auto tag) -> int {
    using T = decltype(tag);
    if (dst_dtype == XRS_DTYPE_F32) return launch<T, float>(a, coord_mode, stream);
    return launch<T, double>(a, coord_mode, stream);
  });
}

}  // namespace xrs
