// te_window_plan.h -- te_run_window_expression (gridMapFilters/SlidingWindowMathExpressionFilter) as a plan: plain C++, no
// HIP, shared with the CPU test (tests/cpu/window_plan_check.cpp).  The window size from the parameters, the window of a
// cell, which route a call and a workgroup take, the LDS of the kernels, and which cell belongs to which workgroup.
//
// The kernels (te_window_expr.hip).  A workgroup of 256 lanes owns kTI x kTJ = 32 x 8 cells (rows are contiguous in memory),
// one cell per lane; the tiles of a map are numbered along the rows first.  Around its cells a workgroup stages the tile with
// a halo of m = (w - 1) / 2 cells in LDS while that fits in kMaxLds beside the operand stacks; otherwise the same walk reads
// global memory.
//   direct      every cell walks its window column by column, once for the inner reductions and once for the outer ones:
//               O(w^2) per cell.  Every program, every edge handling.
//   separable   programs without a nested reduction: pass A leaves the column Partial of rows [i - m, i + m] for every cell
//               row i of the tile and every column of the tile with its halo in LDS, pass B folds the w column partials of a
//               cell in column order: O(w) per cell.  The fold is the contract's own order (rule 5), so the bits are those
//               of the direct route.  Edge handling `mean` pads a clipped window with a value of that window alone: a
//               workgroup one of whose windows is clipped walks its cells directly.
//
// Route by plan (TE_OPT_WINDOW_EXPR_ROUTE = 0): the separable route for every eligible program at w >= kSepMinWindow = 5, the
// direct route below.  Measured on a 4096 x 4096 map with meanOfFinites (tools/window_expression_bench.py):
// separable against direct 0.801 / 0.803 ms at w = 3 (no difference beyond the noise: direct), 0.807 / 0.818 at 5, 0.814 / 1.43
// at 9, 2.13 / 6.48 at 21.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TE_WIN_HD __host__ __device__ inline
#else
#define TE_WIN_HD inline
#endif

namespace te {
namespace wexpr {

constexpr int kTI = 32, kTJ = 8, kThreads = kTI * kTJ;
constexpr size_t kMaxLds = 64 * 1024;  // what a workgroup may take: the figure of te_radius_plan.h and te_median_plan.h
constexpr int kSepMinWindow = 5;  // measured, see above
constexpr int kStackSlots = 7, kResSlots = 4;  // te_expr.h: kMaxStack - 1 (the top stays in a register), kMaxRed
constexpr size_t kBaseLds = (size_t)(kStackSlots + kResSlots) * kThreads * sizeof(float);
constexpr size_t kPartialBytes = sizeof(double) + 2 * sizeof(float) + sizeof(uint32_t);  // one column Partial, as arrays
constexpr int kMaxMapSide = 1 << 30;  // rows, cols and m stay below it: i + m and j + m fit in an int

enum Edge { kInside = 0, kCrop = 1, kEmpty = 2, kMean = 3 };  // TE_EDGE_*
enum Route { kRouteSeparable = 1, kRouteDirect = 2 };

// Rule 2.  0, or the reason as text.
inline const char* window_from_params(int window_size, int use_window_length, double window_length, double resolution, int* w) {
  long long v = window_size;
  if (use_window_length) {
    if (!(window_length >= 0.0) || !isfinite(window_length)) return "window_length must be finite and not negative";
    const double q = round(window_length / resolution);  // half away from zero
    if (!(q < 2147483000.0)) return "window_length is more than 2^31 cells";
    v = (long long)(int)q;
    if (v % 2 == 0) ++v;
  }
  if (v < 1 || v % 2 == 0) return "the window size must be odd and at least 1";
  *w = (int)v;
  return nullptr;
}

// Rule 3: the window of cell (i, j).  W = rows [rlo, rhi] x columns [clo, chi] in map coordinates (beyond the map: the
// padding); B = W clipped to the map.
struct Extent {
  int rlo, rhi, clo, chi;      // W
  int blo, bhi, bclo, bchi;    // B
  bool clipped;                // B != the w x w rectangle
  bool visited;
};
TE_WIN_HD Extent extent(int edge, int m, int rows, int cols, int i, int j, bool centre_finite, bool compute_empty_cells) {
  Extent e;
  e.blo = i - m < 0 ? 0 : i - m;
  e.bhi = i + m > rows - 1 ? rows - 1 : i + m;
  e.bclo = j - m < 0 ? 0 : j - m;
  e.bchi = j + m > cols - 1 ? cols - 1 : j + m;
  e.clipped = i - m < 0 || i + m > rows - 1 || j - m < 0 || j + m > cols - 1;
  const bool padded = edge == kEmpty || edge == kMean;
  e.rlo = padded ? i - m : e.blo;
  e.rhi = padded ? i + m : e.bhi;
  e.clo = padded ? j - m : e.bclo;
  e.chi = padded ? j + m : e.bchi;
  e.visited = !(edge == kInside && e.clipped) && (compute_empty_cells || centre_finite);
  return e;
}

struct Plan {
  int route;          // of the call; a workgroup of the separable route may still walk directly (wg_separable)
  int w, m;
  int tile_in_lds;    // the tile with its halo is staged
  int tile_rows, tile_cols;  // kTI + 2 m, kTJ + 2 m (staged or not)
  size_t lds_bytes;   // dynamic LDS of the launch
  size_t off_tile, off_part;  // byte offsets: the staged tile, the column partials of pass A
  unsigned tiles_i, tiles_j;
  unsigned long long tiles;   // per map: tiles_i * tiles_j, the grid's x
  int fits;           // rows, cols, m and the tile count are within what the kernels index
  // A region call (te_region_plan.h: wexpr::region_plan): the tiles start at (oi0, oj0) instead of the map's corner and own
  // the cells below (oi1, oj1); tiles_i, tiles_j and tiles count the tiles over that rectangle.  The whole-map plan: region 0,
  // the rectangle the map.
  int region;
  int oi0, oj0, oi1, oj1;
};

// option: TE_OPT_WINDOW_EXPR_ROUTE -- 0 by plan, 1 the separable route wherever allowed, 2 the direct route always
inline Plan plan(int rows, int cols, int w, int n_red, int n_outer, int option) {
  Plan p;
  memset(&p, 0, sizeof(p));
  p.w = w;
  p.m = (w - 1) / 2;
  p.tiles_i = (unsigned)((rows + kTI - 1) / kTI);
  p.tiles_j = (unsigned)((cols + kTJ - 1) / kTJ);
  p.tiles = (unsigned long long)p.tiles_i * p.tiles_j;
  p.fits = rows >= 1 && cols >= 1 && rows <= kMaxMapSide && cols <= kMaxMapSide && p.m < kMaxMapSide && p.tiles <= 0x7fffffffull;
  const long long tr = (long long)kTI + 2ll * p.m, tc = (long long)kTJ + 2ll * p.m;
  const bool small = p.m < 65536;  // (tr * tc cannot overflow)
  const long long tile_bytes = small ? tr * tc * (long long)sizeof(float) : (long long)kMaxLds + 1;
  p.tile_rows = small ? (int)tr : 0;
  p.tile_cols = small ? (int)tc : 0;
  p.tile_in_lds = (long long)kBaseLds + tile_bytes <= (long long)kMaxLds;
  p.off_tile = kBaseLds;
  p.off_part = kBaseLds + (p.tile_in_lds ? (size_t)tile_bytes : 0);
  const long long part_bytes = small ? (long long)n_red * kTI * tc * (long long)kPartialBytes : (long long)kMaxLds + 1;
  bool sep = option != 2 && n_red > 0 && n_outer == 0 && p.tile_in_lds && (long long)p.off_part + part_bytes <= (long long)kMaxLds;
  if (option == 0 && w < kSepMinWindow) sep = false;
  p.route = sep ? kRouteSeparable : kRouteDirect;
  p.lds_bytes = sep ? p.off_part + (size_t)part_bytes : p.off_part;
  p.oi1 = rows;
  p.oj1 = cols;
  return p;
}

// the smallest odd window the plan does not stage in LDS
inline int smallest_window_off_lds() {
  int w = 1;
  while (plan(64, 64, w, 1, 0, 2).tile_in_lds) w += 2;
  return w;
}

// A workgroup of the separable route whose tile starts at (i0, j0): `mean` pads a clipped window with that window's own mean,
// so only a workgroup none of whose windows is clipped folds column partials.
TE_WIN_HD bool wg_separable(int edge, int m, int rows, int cols, int i0, int j0) {
  if (edge != kMean) return true;
  const int i1 = i0 + kTI - 1 < rows - 1 ? i0 + kTI - 1 : rows - 1, j1 = j0 + kTJ - 1 < cols - 1 ? j0 + kTJ - 1 : cols - 1;
  return i0 - m >= 0 && i1 + m <= rows - 1 && j0 - m >= 0 && j1 + m <= cols - 1;
}

// Ownership: tile t of a map (blockIdx.x) and lane l (threadIdx.x) own cell (i, j); cells beyond the map have no owner.
TE_WIN_HD void cell_of(unsigned tiles_i, unsigned tile, int lane, int* i, int* j) {
  *i = (int)(tile % tiles_i) * kTI + lane % kTI;
  *j = (int)(tile / tiles_i) * kTJ + lane / kTI;
}
TE_WIN_HD void owner_of(unsigned tiles_i, int i, int j, unsigned* tile, int* lane) {
  *tile = (unsigned)(j / kTJ) * tiles_i + (unsigned)(i / kTI);
  *lane = (j % kTJ) * kTI + i % kTI;
}

// ... of a plan with an origin (a region call): the same numbering over the tiles of [oi0, oi1) x [oj0, oj1); a cell at or
// beyond (oi1, oj1) has no owner.  The whole-map plan has the origin (0, 0): cell_of / owner_of above.
TE_WIN_HD bool cell_of(const Plan& p, unsigned tile, int lane, int* i, int* j) {
  cell_of(p.tiles_i, tile, lane, i, j);
  *i += p.oi0;
  *j += p.oj0;
  return *i < p.oi1 && *j < p.oj1;
}
TE_WIN_HD void owner_of(const Plan& p, int i, int j, unsigned* tile, int* lane) { owner_of(p.tiles_i, i - p.oi0, j - p.oj0, tile, lane); }

// workgroups a call leaves in counts[0] (separable) and counts[1] (direct), per map
inline void expected_counts(const Plan& p, int edge, int rows, int cols, unsigned long long counts[2]) {
  counts[0] = counts[1] = 0;
  for (unsigned t = 0; t < p.tiles; ++t) {
    int i0, j0;
    cell_of(p, t, 0, &i0, &j0);
    ++counts[p.route == kRouteSeparable && wg_separable(edge, p.m, rows, cols, i0, j0) ? 0 : 1];
  }
}

}  // namespace wexpr
}  // namespace te
