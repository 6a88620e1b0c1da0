// xrs_reproject.hpp — what the K1 gathers of xrs_reproject.hip (K1b/K1c/K1p) and
// xrs_reproject_bicubic.hip (K1q and its per-pixel variant) share: the work
// decomposition, the reference's per-axis index math and the row loads.
#pragma once

#include "xrs_common.hpp"

namespace xrs {
namespace k1 {

constexpr int kThreads = 256;
constexpr int kPx = 2;                       // columns per thread
constexpr int kSegW = kThreads * kPx;        // columns per work item
constexpr int kBand = 32;                    // target rows per work item
constexpr int kRows = 8;                     // target rows whose loads are in flight together

// K1b's work shape per output width.  float32 out: 512 columns x 32 rows,
// 8 rows in flight.  float64 out (the reference's bilinear dtype, twice the
// store bytes): 1024 columns x 12 rows, 4 rows in flight — with the round-5
// prologue 2 % faster than the 8-row bands of rounds 3-4 (3.533 vs 3.603-3.615
// ms at config 5, profiles/r05_k1_f64out_shapes_ab.jsonl; 512 x 16 3.56,
// 1024 x 16 3.58, 512 x 32 3.60); each output width takes its own shape
// (profiles/r03_k1_shapes_ab.jsonl).
template <typename O>
struct K1Shape {
  static constexpr int px = sizeof(O) == 8 ? 4 : kPx;
  static constexpr int band = sizeof(O) == 8 ? 12 : kBand;
  static constexpr int rows = sizeof(O) == 8 ? 4 : kRows;
  static constexpr int segw = kThreads * px;
};
constexpr int kRows2D = 2;                   // K1c: target rows per step (2-D tables; 4: slower)

struct AxisEntry {   // one resolved column (or row) of one tile
  int32_t f;         // source index of floor(ix) (nearest: of rint(ix)); -1 = outside source
  int32_t c;         // source index of ceil(ix); -1 = outside source
  double d;          // ix - (double)(int16)floor(ix)
};
static_assert(sizeof(AxisEntry) == 16, "AxisEntry layout");

// coord_mode 2: the source-CRS x of target column c in tile column tx, as the
// host computes it (dask's blockwise linspace of the pixel centres,
// regular.py:44-52, then the separable transformation's scalings,
// reproject.py:472-496): v = k == n-1 ? stop : k * step + start (k = c - tx *
// tile_w), x = (v * m1) * m2.  src_x then holds ntiles_x records followed by
// (m1, m2); the host uses this mode only after checking it bit for bit.
struct ColumnGen {
  double start, stop, step, n;
};
static_assert(sizeof(ColumnGen) == 32, "ColumnGen layout");

struct Geometry {
  int64_t src_h, src_w, src_row0, src_rows;
  int64_t dst_h, dst_w, row_begin, row_end;
  int64_t tile_h, tile_w, ntiles_x, ntiles_y;
  const double* src_x;
  const double* src_y;
  const float* tile_x0;
  const float* tile_y0;
  const int64_t* tile_win;
  int64_t win_h, win_w;
  double x_res, neg_y_res;
  int32_t* err_flags;
  int64_t band;   // target rows per work item of the gathers
  int64_t segw;   // target columns per work item (kThreads x columns per thread)
  int64_t band_first;   // bands of tile row ty0 above row_begin (not in the work list)
  int64_t xgen;         // K1b: src_x holds column generators (coord_mode 2, ColumnGen)
};

// numpy fancy index on a window axis of length `win` with an int16 index:
// negative indices wrap once (python semantics), anything else outside
// [0, win) is an IndexError (reproject.py:284,292-295,322-325).
__device__ inline bool window_index(int16_t idx16, int64_t win, int64_t& out) {
  int64_t i = idx16;
  if (i < 0) i += win;
  out = i;
  return i >= 0 && i < win;
}

// Window position -> source index along one axis; -1 when the window position
// lies in the constant-padded region (outside the source).  Rows are returned
// relative to the band held on this device.
__device__ inline int32_t to_source(int64_t w0, int64_t widx, int64_t size, int64_t band0,
                                    int64_t band_len, int32_t& eflags) {
  const int64_t g = w0 + widx;
  if (g < 0 || g >= size) return -1;
  const int64_t l = g - band0;
  if (l < 0 || l >= band_len) {
    eflags |= XRS_EFLAG_BAND;
    return -1;
  }
  return (int32_t)l;
}

// The reference's index math for one coordinate along one axis
// (reproject.py:278-283 nearest, 286-291 / 316-321 floor/ceil/diff).
template <int INTERP>
__device__ inline AxisEntry resolve_axis(double coord, float origin, double res, int64_t win,
                                         int64_t w0, int64_t size, int64_t band0,
                                         int64_t band_len, int32_t& eflags) {
  const double i = (coord - (double)origin) / res;
  AxisEntry e;
  if (INTERP == XRS_INTERP_NEAREST) {
    int64_t wi;
    if (window_index(f64_to_i16_np(rint(i)), win, wi)) {
      e.f = to_source(w0, wi, size, band0, band_len, eflags);
    } else {
      eflags |= XRS_EFLAG_INDEX;
      e.f = -1;
    }
    e.c = e.f;
    e.d = 0.0;
  } else {
    const int16_t fi = f64_to_i16_np(floor(i)), ci = f64_to_i16_np(ceil(i));
    e.d = i - (double)fi;
    int64_t wf, wc;
    const bool okf = window_index(fi, win, wf);
    const bool okc = window_index(ci, win, wc);
    if (!okf || !okc) eflags |= XRS_EFLAG_INDEX;
    e.f = okf ? to_source(w0, wf, size, band0, band_len, eflags) : -1;
    e.c = okc ? to_source(w0, wc, size, band0, band_len, eflags) : -1;
  }
  return e;
}

// resolve_axis for the per-pixel gathers (K1c, K1p): the same entries with
// 32-bit index arithmetic whenever every quantity fits (window and band
// bounds below 2^30, |window origin| <= 2^30: no sum or difference below can
// leave int32); otherwise resolve_axis itself.
template <int INTERP>
__device__ inline AxisEntry resolve_axis_px(double coord, float origin, double res, int64_t win,
                                            int64_t w0, int64_t size, int64_t band0,
                                            int64_t band_len, int32_t& eflags) {
  constexpr int64_t kLim = int64_t(1) << 30;
  if (!(win <= kLim && size <= INT32_MAX && band0 >= 0 && band0 <= kLim && band_len <= INT32_MAX &&
        w0 >= -kLim && w0 <= kLim))
    return resolve_axis<INTERP>(coord, origin, res, win, w0, size, band0, band_len, eflags);
  const int32_t win32 = (int32_t)win, w032 = (int32_t)w0, size32 = (int32_t)size;
  const int32_t b032 = (int32_t)band0, bl32 = (int32_t)band_len;
  auto window32 = [&](int16_t idx16, int32_t& out) {
    int32_t i = idx16;
    if (i < 0) i += win32;
    out = i;
    return i >= 0 && i < win32;
  };
  auto source32 = [&](int32_t widx) -> int32_t {
    const int32_t g = w032 + widx;
    if (g < 0 || g >= size32) return -1;
    const int32_t l = g - b032;
    if (l < 0 || l >= bl32) {
      eflags |= XRS_EFLAG_BAND;
      return -1;
    }
    return l;
  };
  const double i = (coord - (double)origin) / res;
  AxisEntry e;
  if (INTERP == XRS_INTERP_NEAREST) {
    int32_t wi;
    if (window32(f64_to_i16_np(rint(i)), wi)) {
      e.f = source32(wi);
    } else {
      eflags |= XRS_EFLAG_INDEX;
      e.f = -1;
    }
    e.c = e.f;
    e.d = 0.0;
  } else {
    const int16_t fi = f64_to_i16_np(floor(i)), ci = f64_to_i16_np(ceil(i));
    e.d = i - (double)fi;
    int32_t wf, wc;
    const bool okf = window32(fi, wf);
    const bool okc = window32(ci, wc);
    if (!okf || !okc) eflags |= XRS_EFLAG_INDEX;
    e.f = okf ? source32(wf) : -1;
    e.c = okc ? source32(wc) : -1;
  }
  return e;
}

// ---- interpolation of one pixel (reproject.py:304-314, 326-328) ------------
template <typename T, int INTERP>
__device__ inline double interp4(T v00, T v01, T v10, T v11, double dx, double dy) {
  if (INTERP == XRS_INTERP_BILINEAR) {
    const double u0 = Conv<T>::to_f64(v00) + dx * Conv<T>::to_f64(Conv<T>::diff(v01, v00));
    const double u1 = Conv<T>::to_f64(v10) + dx * Conv<T>::to_f64(Conv<T>::diff(v11, v10));
    return u0 + dy * (u1 - u0);
  }
  if (dx + dy < 1.0)  // closest triangle
    return Conv<T>::to_f64(v00) + dx * Conv<T>::to_f64(Conv<T>::diff(v01, v00)) +
           dy * Conv<T>::to_f64(Conv<T>::diff(v10, v00));
  return Conv<T>::to_f64(v11) + (1.0 - dx) * Conv<T>::to_f64(Conv<T>::diff(v10, v11)) +
         (1.0 - dy) * Conv<T>::to_f64(Conv<T>::diff(v01, v11));
}

// A wave-uniform source row as a buffer resource (4 SGPRs): its taps are
// buffer loads with a 32-bit lane byte offset — no 64-bit address per lane
// (VALU and VGPRs the 16 tap rows of a batch no longer pay)
__device__ inline __amdgpu_buffer_rsrc_t row_rsrc(const void* row, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(row), 0, (int)bytes, 0x00020000);
}
template <typename T>
__device__ inline T row_at(__amdgpu_buffer_rsrc_t rs, uint32_t off) {
  if constexpr (sizeof(T) == 1) {
    return __builtin_bit_cast(T, (uint8_t)__builtin_amdgcn_raw_buffer_load_b8(rs, off, 0, 0));
  } else if constexpr (sizeof(T) == 2) {
    return __builtin_bit_cast(T, (uint16_t)__builtin_amdgcn_raw_buffer_load_b16(rs, off, 0, 0));
  } else if constexpr (sizeof(T) == 4) {
    return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0));
  } else {
    return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 0));
  }
}

struct GatherArgs {
  Geometry g;
  const void* src;
  int64_t n, src_sn, src_sy;
  void* dst;
  int64_t dst_sn, dst_sy;
  double fill;
};

// Work decomposition shared by K1b/K1c: bands of kBand rows inside one tile row
// x segments of kSegW columns inside one tile column, band-major; the XCDs
// take whole bands in turn (XCD x: bands x, x + 8, ...).  The list starts at
// the band holding row_begin and ends at the band holding row_end - 1, so a
// row band of the raster (a rank's share) has no empty items (blocks are dealt
// to XCDs round-robin whatever their cost: empty items would idle an XCD).
// Returns false for empty items (partial edge tiles).
struct WorkItem {
  int64_t t, ty, tx, r0, r1, c0, c1;
};
__device__ inline bool work_item(const Geometry& g, int64_t w, int64_t ty0, int64_t nsegs,
                                 int64_t bands_per_tile, int64_t segs_per_tile, WorkItem& it) {
  const int64_t bw = w / nsegs, s = w - bw * nsegs;
  const int64_t b = bw + g.band_first;
  const int64_t tyi = b / bands_per_tile;
  it.ty = ty0 + tyi;
  const int64_t bi = b - tyi * bands_per_tile;
  const int64_t tr0 = it.ty * g.tile_h;
  it.r0 = max(g.row_begin, tr0 + bi * g.band);
  it.r1 = min(min(g.row_end, tr0 + g.tile_h), tr0 + bi * g.band + g.band);
  it.tx = s / segs_per_tile;
  const int64_t si = s - it.tx * segs_per_tile;
  it.c0 = it.tx * g.tile_w + si * g.segw;
  it.c1 = min(min(g.dst_w, it.tx * g.tile_w + g.tile_w), it.c0 + g.segw);
  it.t = it.ty * g.ntiles_x + it.tx;
  return it.r0 < it.r1 && it.c0 < it.c1;
}

// Work decomposition of the gathers (K1b/K1c/K1p): bands from the one holding
// row_begin to the one holding row_end - 1, all segments of a band together.
struct Work {
  GatherArgs args;
  int64_t ty0, ty1, nsegs, bands_per_tile, segs_per_tile, nwork;
  int nb;
};
inline Work work_of(const GatherArgs& a, int64_t band = kBand, int64_t segw = kSegW) {
  const Geometry& g = a.g;
  Work k;
  k.args = a;
  k.ty0 = g.row_begin / g.tile_h;
  k.ty1 = (g.row_end - 1) / g.tile_h + 1;
  // band height / grid cap: fixed in the product; xrs_testing_set() can change
  // them so the tests cover items that split tiles and the grid-stride loop
  const int64_t band_knob = xrs_testing_value(XRS_TESTING_REPROJECT_BAND);
  k.args.g.band = band_knob > 0 ? band_knob : band;
  k.args.g.segw = segw;
  k.bands_per_tile = (g.tile_h + k.args.g.band - 1) / k.args.g.band;
  k.segs_per_tile = (g.tile_w + k.args.g.segw - 1) / k.args.g.segw;
  k.nsegs = g.ntiles_x * k.segs_per_tile;
  k.args.g.band_first = (g.row_begin - k.ty0 * g.tile_h) / k.args.g.band;
  const int64_t band_last = (k.ty1 - 1 - k.ty0) * k.bands_per_tile +
                            (g.row_end - 1 - (k.ty1 - 1) * g.tile_h) / k.args.g.band;
  k.nwork = (band_last - k.args.g.band_first + 1) * k.nsegs;
  // One work item per block (measured fastest: short blocks let the dispatcher
  // balance the CUs and keep each XCD's concurrent row set L2-sized; a
  // persistent grid of 8 blocks/CU was 12 % slower).
  const int64_t bpc = xrs_testing_value(XRS_TESTING_REPROJECT_BLOCKS_PER_CU);
  k.nb = grid_blocks(k.nwork, 1, bpc > 0 ? (int)(256 * bpc) : (1 << 24));
  return k;
}

// n / d for n < 2^31 by a multiply-high (the round-up method: m = floor(2^32
// (2^l - d) / d) + 1, l = ceil(log2 d); exact for every such n and d >= 1)
struct DivU32 {
  uint32_t m, l;
  static DivU32 make(uint32_t d) {
    uint32_t l = 0;
    while ((1ull << l) < d) ++l;
    return DivU32{(uint32_t)((((1ull << l) - d) << 32) / d + 1), l};
  }
  __device__ uint32_t div(uint32_t n) const { return (__umulhi(n, m) + n) >> l; }
};

// XRS_INTERP_BICUBIC (xrs_reproject_bicubic.hip): K1q for the separable
// coord_modes, the per-pixel 16-tap gather for coord_mode 1; dst_dtype is
// float32 or float64 (checked by the caller)
int launch_bicubic(const GatherArgs& a, int src_dtype, int dst_dtype, int coord_mode,
                   hipStream_t stream);

// XRS_INTERP_BICUBIC under xrs_reproject_proj (xrs_reproject_proj_bicubic.hip):
// K1pq, the projection per pixel and a patch's source rectangle staged in LDS;
// the pipeline kinds k0, k1 (0: no step) and dst_dtype (float32 or float64)
// are checked by the caller
int launch_proj_bicubic(const GatherArgs& a, const XrsProjStep& s0, const XrsProjStep& s1, int k0,
                        int k1, int src_dtype, int dst_dtype, hipStream_t stream);

}  // namespace k1
}  // namespace xrs
