// xrs_coords.hip — K8: the full-raster analysis of 2-D coordinates for gfx950.
//
// K8 coords_stats replaces the two passes of new_grid_mapping_from_coords'
// 2-D branch that read every coordinate (gridmapping/coords.py:99-327):
// `any(x > 180)` and the positive cell-area extremes of
// _estimate_2d_resolution (coords.py:226-264: four np.diff, four
// concatenations, two square roots, the geographic cosine, nanargmin /
// nanargmax — a dozen full-size temporaries in numpy).  One pass over x and y,
// 16 B per point.
//
// Work shape (K4's): a wave takes a block of kRows source rows x 64 columns,
// lane l column l; the grid is the resident blocks and each wave walks several
// blocks.  Per block the wave loads its kRows rows and one halo row (the row
// below the block), all loads issued before the first is consumed; the row
// below a pixel is the next register of the column, the right-hand neighbour
// comes from lane l + 1 by DPP.  Lane 63's neighbour (first column of the next
// column block) and the last column's (column w - 2, see below) are loaded by
// those lanes alone.  The coordinates are read (kRows + 1) / kRows = 1.06x.
//
// Edges, as the reference's concatenations: the last column repeats column
// w - 2's x-direction difference and the last row repeats row h - 2's
// y-direction difference.  |a - b| = |b - a| exactly, so the last column takes
// column w - 2 as its "right-hand" neighbour and the last row takes row h - 2
// as its "row below": no special case in the arithmetic.
//
// Reduction: (area, flat index) pairs, equal areas resolve to the lowest index
// (numpy's nanargmin / nanargmax return the first).  Per lane in registers,
// per wave by DPP steps (as K4's wave extremes; no ds_bpermute butterflies),
// per block through LDS, and every block writes one partial record with plain
// vector stores.  A second one-block kernel folds the records (a float64
// atomic min on the value could not break index ties).
//
// The library is compiled with -ffp-contract=off: the projected-mode areas are
// numpy's bit for bit (IEEE add, multiply, square root); geographic mode
// differs by the device cosine.

#include <math.h>

#include "xrs_common.hpp"

namespace xrs {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRows = 16;          // rows of a wave's block (K4's kBoxBlockRows)
constexpr int kMaxBlocks = 4096;   // bound of the grid = records of the workspace
constexpr double kDegToRad = 3.141592653589793238462643383279502884 / 180.0;  // np.radians
constexpr double kEarthRadius = 6371000.0;

static_assert(sizeof(XrsCoordsStats) == 48, "XrsCoordsStats is 48 bytes (include/xrs.h)");

struct CoordsArgs {
  const double* x;
  const double* y;
  int64_t h, w, sy;
  XrsCoordsStats* part;   // (gridDim.x) partial records
};

struct Ext {     // a candidate extreme: area and flat index
  double v;
  int64_t i;
};

// the better of two candidates; equal areas: the lower index
template <bool MAX>
__device__ inline Ext better(Ext a, Ext b) {
  const bool take = (MAX ? b.v > a.v : b.v < a.v) || (b.v == a.v && b.i < a.i);
  // (member-wise: `take ? b : a` selects between two addresses and puts both on the stack)
  return Ext{take ? b.v : a.v, take ? b.i : a.i};
}

template <int CTRL, int ROWS>
__device__ inline uint64_t dpp_keep_u64(uint64_t b) {   // unwritten lanes keep their value
  const int lo = (int)(uint32_t)b, hi = (int)(uint32_t)(b >> 32);
  const uint32_t l = (uint32_t)__builtin_amdgcn_update_dpp(lo, lo, CTRL, ROWS, 0xF, false);
  const uint32_t h = (uint32_t)__builtin_amdgcn_update_dpp(hi, hi, CTRL, ROWS, 0xF, false);
  return ((uint64_t)h << 32) | l;
}
template <int CTRL, int ROWS>
__device__ inline Ext dpp_keep(const Ext& e) {
  return Ext{__longlong_as_double((int64_t)dpp_keep_u64<CTRL, ROWS>(
                 (uint64_t)__double_as_longlong(e.v))),
             (int64_t)dpp_keep_u64<CTRL, ROWS>((uint64_t)e.i)};
}
__device__ inline uint64_t readlane_u64(uint64_t b, int lane) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), lane);
  return ((uint64_t)hi << 32) | lo;
}

// Wave extreme of (area, index), wave-uniform result: each quad, half-row and
// row of 16 lanes, then rows 0+1 / 2+3 and all four into lane 63 (the DPP
// steps of K4's wave_ext_f64, on pairs).
template <bool MAX>
__device__ inline Ext wave_best(Ext e) {
  e = better<MAX>(e, dpp_keep<0xB1, 0xF>(e));    // quad_perm [1, 0, 3, 2]
  e = better<MAX>(e, dpp_keep<0x4E, 0xF>(e));    // quad_perm [2, 3, 0, 1]
  e = better<MAX>(e, dpp_keep<0x141, 0xF>(e));   // row_half_mirror
  e = better<MAX>(e, dpp_keep<0x140, 0xF>(e));   // row_mirror
  e = better<MAX>(e, dpp_keep<0x142, 0xA>(e));   // row_bcast:15 -> rows 1, 3
  e = better<MAX>(e, dpp_keep<0x143, 0xC>(e));   // row_bcast:31 -> rows 2, 3
  return Ext{__longlong_as_double((int64_t)readlane_u64((uint64_t)__double_as_longlong(e.v), 63)),
             (int64_t)readlane_u64((uint64_t)e.i, 63)};
}

__device__ inline double dpp_next_f64(double v) {   // lane i <- lane i + 1 (lane 63: 0)
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)b, 0x130, 0xF, 0xF, true);
  const uint32_t hi =
      (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)(b >> 32), 0x130, 0xF, 0xF, true);
  return __longlong_as_double((int64_t)(((uint64_t)hi << 32) | lo));
}

// _abs_no_nan (coords.py:335-337): |d|, with NaN and np.isclose(|d|, 0)
// (|d| <= 1e-8, numpy's default atol against 0) counted as 0; inf stays inf
__device__ inline double abs_no_nan(double d) {
  d = fabs(d);
  return d > 1e-8 ? d : 0.0;
}

template <bool GEO>
__device__ inline double cell_area(double dxx, double dxy, double dyx, double dyy) {
  double ax = sqrt(dxx * dxx + dxy * dxy);
  double ay = sqrt(dyx * dyx + dyy * dyy);
  if (GEO) {   // coords.py:250-254
    const double xr = ax * kDegToRad, yr = ay * kDegToRad;
    ax = (kEarthRadius * cos(xr)) * yr;
    ay = kEarthRadius * yr;
  }
  return ax * ay;
}

struct Fold {    // extremes, count and flag of a lane / wave / block
  Ext mn, mx;
  int64_t npos;
  bool gt;
};
__device__ inline Fold fold_init() {
  return Fold{Ext{INFINITY, INT64_MAX}, Ext{0.0, INT64_MAX}, 0, false};
}
// (records are read and written field by field: a whole-struct copy goes
// through a stack temporary, i.e. scratch memory)
__device__ __forceinline__ void fold_record(Fold& f, const XrsCoordsStats* r) {
  f.mn = better<false>(f.mn, Ext{r->area_min, r->idx_min});
  f.mx = better<true>(f.mx, Ext{r->area_max, r->idx_max});
  f.npos += r->n_positive;
  f.gt = f.gt || r->any_gt_180 != 0;
}
__device__ __forceinline__ void store_record(XrsCoordsStats* r, const Fold& f) {
  r->area_min = f.mn.v;
  r->area_max = f.mx.v;
  r->idx_min = f.mn.i;
  r->idx_max = f.mx.i;
  r->n_positive = f.npos;
  r->any_gt_180 = f.gt ? 1 : 0;
  r->pad = 0;
}

template <bool GEO>
__global__ void __launch_bounds__(kThreads)
coords_stats_kernel(CoordsArgs a) {
  __shared__ XrsCoordsStats swave[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t ncb = (a.w + 63) / 64, nrb = (a.h + kRows - 1) / kRows;
  const int64_t nblk = ncb * nrb;
  const int64_t nwaves = (int64_t)gridDim.x * kWaves;
  Fold f = fold_init();   // npos is wave-uniform (ballot counts)
  for (int64_t blk = (int64_t)blockIdx.x * kWaves + wave; blk < nblk; blk += nwaves) {
    const int64_t rb = blk / ncb, cb = blk - rb * ncb;   // wave-uniform
    const int64_t j0 = rb * kRows, i = cb * 64 + lane;
    const bool col_ok = i < a.w;
    const int nrows = (int)min((int64_t)kRows, a.h - j0);
    // the lanes whose right-hand neighbour no lane of the wave holds
    const bool edge = col_ok && (lane == 63 || i == a.w - 1);
    const int64_t ie = i + 1 < a.w ? i + 1 : a.w - 2;
    double x[kRows + 1], y[kRows + 1], xe[kRows], ye[kRows];
#pragma unroll
    for (int s = 0; s <= kRows; ++s) {
      x[s] = y[s] = NAN;
      if (s < kRows) xe[s] = ye[s] = NAN;
      // slot nrows is the row below the block, for the last row: row h - 2.
      // (The slots after it, of the last row block only, read row h - 2
      // again and are not used: no branch between the loads.)
      const int64_t o = (j0 + s < a.h ? j0 + s : a.h - 2) * a.sy;
      if (col_ok) {
        x[s] = a.x[o + i];
        y[s] = a.y[o + i];
      }
      if (s < kRows && edge) {
        xe[s] = a.x[o + ie];
        ye[s] = a.y[o + ie];
      }
    }
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      if (r < nrows) {   // wave-uniform: every lane takes part in the DPP moves
        double xn = dpp_next_f64(x[r]), yn = dpp_next_f64(y[r]);
        if (edge) {
          xn = xe[r];
          yn = ye[r];
        }
        const double area = cell_area<GEO>(abs_no_nan(xn - x[r]), abs_no_nan(x[r + 1] - x[r]),
                                           abs_no_nan(yn - y[r]), abs_no_nan(y[r + 1] - y[r]));
        const bool pos = col_ok && area > 0.0;
        f.npos += __builtin_popcountll(__ballot(pos));
        if (pos) {
          const Ext e{area, (j0 + r) * a.w + i};
          f.mn = better<false>(f.mn, e);
          f.mx = better<true>(f.mx, e);
        }
        f.gt = f.gt || x[r] > 180.0;   // (NaN where there is no pixel)
      }
    }
  }
  f.mn = wave_best<false>(f.mn);
  f.mx = wave_best<true>(f.mx);
  f.gt = __ballot(f.gt) != 0;
  if (lane == 0) store_record(&swave[wave], f);
  __syncthreads();
  if (threadIdx.x == 0) {
    Fold b = fold_init();
#pragma unroll
    for (int k = 0; k < kWaves; ++k) fold_record(b, &swave[k]);
    store_record(&a.part[blockIdx.x], b);
  }
}

// The partial records of K8's blocks folded into the result record (one block).
__global__ void __launch_bounds__(kThreads)
coords_stats_fold_kernel(const XrsCoordsStats* part, int n, XrsCoordsStats* out) {
  __shared__ XrsCoordsStats swave[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Fold f = fold_init();
  for (int k = threadIdx.x; k < n; k += kThreads) fold_record(f, &part[k]);
  f.mn = wave_best<false>(f.mn);
  f.mx = wave_best<true>(f.mx);
  f.gt = __ballot(f.gt) != 0;
  // the wave's count: lane counts summed through LDS (64-bit, no DPP carry chain)
  __shared__ unsigned long long scount[kWaves];
  if (lane == 0) scount[wave] = 0;
  __syncthreads();
  if (f.npos != 0) atomicAdd(&scount[wave], (unsigned long long)f.npos);
  __syncthreads();
  f.npos = (int64_t)scount[wave];
  if (lane == 0) store_record(&swave[wave], f);
  __syncthreads();
  if (threadIdx.x == 0) {
    Fold b = fold_init();
#pragma unroll
    for (int k = 0; k < kWaves; ++k) fold_record(b, &swave[k]);
    if (b.npos == 0) {   // no positive area: numpy's all-NaN slice
      b.mn = b.mx = Ext{NAN, -1};
    }
    store_record(out, b);
  }
}

inline int64_t block_count(int64_t h, int64_t w) {   // wave blocks of an (h, w) raster
  return ((w + 63) / 64) * ((h + kRows - 1) / kRows);
}

}  // namespace
}  // namespace xrs

extern "C" int64_t xrs_coords_stats_workspace_size(int64_t h, int64_t w) {
  using namespace xrs;
  if (h < 2 || w < 2 || h > INT32_MAX || w > INT32_MAX) return 0;
  return (int64_t)grid_blocks(block_count(h, w), kWaves, kMaxBlocks) *
         (int64_t)sizeof(XrsCoordsStats);
}

extern "C" int xrs_coords_stats(const double* x, const double* y, int64_t h, int64_t w,
                                int64_t row_stride, int geographic, XrsCoordsStats* out,
                                void* ws, int64_t ws_bytes, void* stream) {
  using namespace xrs;
  if (!x || !y || !out || !ws || h < 2 || w < 2 || h > INT32_MAX || w > INT32_MAX ||
      row_stride < w || row_stride > INT32_MAX ||
      (reinterpret_cast<uintptr_t>(ws) & 7) != 0 || (reinterpret_cast<uintptr_t>(out) & 7) != 0 ||
      ws_bytes < xrs_coords_stats_workspace_size(h, w)) {
    xrs_set_error("xrs_coords_stats: invalid argument (h, w >= 2, row_stride >= w, an 8-byte "
                  "aligned workspace of xrs_coords_stats_workspace_size bytes)");
    return XRS_ERR_ARG;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const void* kernel = geographic ? reinterpret_cast<const void*>(coords_stats_kernel<true>)
                                  : reinterpret_cast<const void*>(coords_stats_kernel<false>);
  // as many blocks as are resident at once, each wave walking its blocks in
  // turn (K4's grid); never more than the workspace holds records for
  const int nres = resident_blocks(kernel, kThreads);
  const int nb = grid_blocks(block_count(h, w), kWaves, nres < kMaxBlocks ? nres : kMaxBlocks);
  CoordsArgs a{x, y, h, w, row_stride, static_cast<XrsCoordsStats*>(ws)};
  if (geographic)
    hipLaunchKernelGGL(coords_stats_kernel<true>, dim3(nb), dim3(kThreads), 0, st, a);
  else
    hipLaunchKernelGGL(coords_stats_kernel<false>, dim3(nb), dim3(kThreads), 0, st, a);
  XRS_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(coords_stats_fold_kernel, dim3(1), dim3(kThreads), 0, st,
                     static_cast<const XrsCoordsStats*>(ws), nb, out);
  XRS_HIP_CHECK(hipGetLastError());
  return XRS_OK;
}
