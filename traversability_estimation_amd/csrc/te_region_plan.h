// te_region_plan.h -- te_run_median_fill_region, te_run_radius_filter_region and te_run_window_expression_region as plans: plain
// C++, no HIP, shared with the CPU tests (tests/cpu/region_plan_check.cpp, tests/cpu/window_region_check.cpp).  How far a
// changed cell of the input reaches into the output, the rectangle a region call writes, the rectangle every mask stage of the fill computes and reads, and the launch geometry of every route
// over that rectangle.  The launchers (te_median_api.hip, te_radius_api.hip) decide nothing of their own.
//
// A region call recomputes every cell of `out` from the input as it is now; it never reads the output layer.  `out` is the
// dirty rectangle grown by the reach and clamped to the map, so the cells it leaves alone cannot have changed.
//
// Reach of the fill (Chebyshev): a changed cell changes V there; k erosions and k dilations of 3 x 3 carry that 2 k cells;
// the window OR carries it r_fill further: the mask changes within r_fill + 2 k.  A median reads r_fill (a hole) or r_existing
// (a finite cell, with filter_existing_values) around its cell.  reach = max(r_fill + 2 k, r_existing).
// The mask stages run in map coordinates on scratch of the map's size, each on the rectangle the next one reads:
//   stage 0       V            on out grown by g = r_fill + 2 k
//   stage s       s-th morph   on out grown by g - s          (s = 1 .. 2 k; reads stage s - 1 within 1 cell, clamped to the MAP:
//                              the region border is no map border, cells outside the map do not vote)
//   row OR        along i      on out grown by r_fill along j only (reads stage 2 k within r_fill along i)
//   column OR     along j      on out                          -> the stored fill mask
// Every rectangle is clamped to the map, and clamp(clamp(x grown a) grown 1) lies in clamp(x grown a + 1): a stage reads
// only what the stage before wrote.
//
// Reach of the radius filters: that of the disc table (te_disc_table.h: the largest |offset| of runs and ties); the disc is
// symmetric, so a cell reads and is read within the same distance.
//
// Launch geometry: the kernels of the whole-map calls with a tile origin and an end of the cells they own -- a workgroup's
// tile starts at out's corner instead of the map's.  For the sliding Mean that is another tiling than the whole-map call's;
// its workgroups decide order_free() over what THEY read, and a sum that passes is the exact real sum, so the bits agree.
#pragma once
#include "te_median_plan.h"
#include "te_radius_plan.h"
#include "te_window_plan.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TE_REGION_HD __host__ __device__ inline
#else
#define TE_REGION_HD inline
#endif

namespace te {
namespace region {

// cells [i0, i1) x [j0, j1); i along the rows (contiguous in memory)
struct Rect {
  int i0, j0, i1, j1;
};
TE_REGION_HD int height(const Rect& r) { return r.i1 - r.i0; }
TE_REGION_HD int width(const Rect& r) { return r.j1 - r.j0; }
TE_REGION_HD size_t cells(const Rect& r) { return (size_t)height(r) * (size_t)width(r); }
// the k-th cell of a rectangle, rows fastest; k < cells(r)
TE_REGION_HD void cell_of(const Rect& r, size_t k, int* i, int* j) {
  const size_t h = (size_t)height(r);
  *i = r.i0 + (int)(k % h);
  *j = r.j0 + (int)(k / h);
}
inline bool inside(const Rect& a, const Rect& b) { return a.i0 >= b.i0 && a.j0 >= b.j0 && a.i1 <= b.i1 && a.j1 <= b.j1; }

// the rectangle checks of te_run_chain_region
inline bool valid_rect(int rows, int cols, int row0, int col0, int h, int w) {
  return row0 >= 0 && col0 >= 0 && h > 0 && w > 0 && h <= rows - row0 && w <= cols - col0;
}
// grown by `by_i` rows and `by_j` columns on both sides, clamped to the map; by_* >= 0 of any size
inline Rect grown(const Rect& r, long long by_i, long long by_j, int rows, int cols) {
  Rect g;
  g.i0 = (long long)r.i0 - by_i < 0 ? 0 : (int)(r.i0 - by_i);
  g.j0 = (long long)r.j0 - by_j < 0 ? 0 : (int)(r.j0 - by_j);
  g.i1 = (long long)r.i1 + by_i > rows ? rows : (int)(r.i1 + by_i);
  g.j1 = (long long)r.j1 + by_j > cols ? cols : (int)(r.j1 + by_j);
  return g;
}

}  // namespace region

namespace median {

// r_exist < 0: finite cells keep their values
inline long long region_reach(int r_fill, int r_exist, int iterations) {
  const long long m = (long long)r_fill + 2ll * (long long)iterations;
  return r_exist > m ? (long long)r_exist : m;
}

struct RegionPlan {
  long long reach;
  region::Rect out;  // the cells written: layer and stored mask
  int r_fill, iterations;
  int rows, cols;
  Plan k;             // route, halo, LDS and the tile grid OVER `out` (blocks: of one map)
  size_t any_blocks;  // general route: counts over the cells of `out`, 256 each
};

// stage s of the mask (0: V, 1 .. 2 k: the morphs) is computed on this rectangle
inline region::Rect mask_stage_rect(const RegionPlan& p, int s) {
  const long long g = (long long)p.r_fill + 2ll * (long long)p.iterations - (long long)s;
  return region::grown(p.out, g, g, p.rows, p.cols);
}
// ... and what it reads of the stage before (s >= 1)
inline region::Rect mask_stage_reads(const RegionPlan& p, int s) { return region::grown(mask_stage_rect(p, s), 1, 1, p.rows, p.cols); }
// the OR along the rows: computed on / reads
inline region::Rect row_or_rect(const RegionPlan& p) { return region::grown(p.out, 0, p.r_fill, p.rows, p.cols); }
inline region::Rect row_or_reads(const RegionPlan& p) { return region::grown(row_or_rect(p), p.r_fill, 0, p.rows, p.cols); }
// the OR along the columns is computed on `out` and reads
inline region::Rect col_or_reads(const RegionPlan& p) { return region::grown(p.out, 0, p.r_fill, p.rows, p.cols); }
// the cells of the input layer a median may read (its window is clamped to the map)
inline region::Rect median_reads(const RegionPlan& p) { return region::grown(p.out, p.k.r, p.k.r, p.rows, p.cols); }

// `dirty` lies in the map (region::valid_rect).  option: TE_OPT_MEDIAN_ROUTE, as plan()
inline RegionPlan region_plan(int rows, int cols, int r_fill, int r_exist, int iterations, int option, const region::Rect& dirty) {
  RegionPlan p;
  p.reach = region_reach(r_fill, r_exist, iterations);
  p.out = region::grown(dirty, p.reach, p.reach, rows, cols);
  p.r_fill = r_fill;
  p.iterations = iterations;
  p.rows = rows;
  p.cols = cols;
  p.k = plan(region::height(p.out), region::width(p.out), 1, r_fill > r_exist ? r_fill : r_exist, option);
  p.any_blocks = (region::cells(p.out) + 255) / 256;
  return p;
}

// the cell a lane of the tile kernel owns: tile (tx, ty) of the grid over `out`, cell (li, lj) of the tile; false: none
inline bool tile_owner(const RegionPlan& p, int tx, int ty, int li, int lj, int* i, int* j) {
  *i = p.out.i0 + tx * kTileRows + li;
  *j = p.out.j0 + ty * kTileCols + lj;
  return *i < p.out.i1 && *j < p.out.j1;
}

}  // namespace median

namespace radius {

struct RegionPlan {
  int reach;
  region::Rect out;
  Plan k;  // the whole-map plan's route, LDS, segment and predicate; the grid OVER `out`
};

// option: TE_OPT_RADIUS_ROUTE, as plan().  The route is the whole-map call's.
inline RegionPlan region_plan(int op, int rows, int cols, const Shape& s, int option, const region::Rect& dirty) {
  RegionPlan p;
  p.reach = s.reach;
  p.out = region::grown(dirty, s.reach, s.reach, rows, cols);
  p.k = plan(op, rows, cols, s, option);
  const int h = region::height(p.out), w = region::width(p.out);
  p.k.grid_x = (unsigned)((h + kTX - 1) / kTX);
  if (p.k.route == kRouteSlide) {
    p.k.grid_y = (unsigned)((w + kTY - 1) / kTY);  // (<= the whole map's, which plan() held against kMaxGridY)
  } else {
    const unsigned g4 = (unsigned)((w + kWaves - 1) / kWaves);
    p.k.grid_y = g4 > kMaxGridY ? kMaxGridY : g4;
  }
  return p;
}

}  // namespace radius

// te_run_window_expression_region.  Reach (Chebyshev): m = (w - 1) / 2 under every edge handling.  A cell reads its window W
// (rule 3 of the contract), which lies within m of the cell.  `inside` and `crop` clip W to the map, `empty` pads it with NaN:
// nothing else is read.  `mean` pads a clipped window with meanOfFinites(B), and B = W clipped to the map lies inside W: the
// padding of a cell reads no cell farther than m either (tests/test_window_region_ref.py holds the reference to exactly
// this).  The visit rule reads the cell's own input (compute_empty_cells) and the map's size.  So a cell farther than m from
// every changed cell keeps its bits, and `out` = the dirty rectangle grown by m, clamped to the map.
// Launch geometry: the kernel of the whole-map call, the tiling started at out's corner; a workgroup stages its tile with the
// halo of m cells as before, every read checked against the MAP (the region border is no map border).  The route, the LDS
// layout and the staging decision are the whole-map plan's.
namespace wexpr {

struct RegionPlan {
  int reach;         // m
  region::Rect out;  // the cells written
  Plan k;            // the whole-map plan with the origin and the end of the owned cells; tiles over `out`
};

// `dirty` lies in the map (region::valid_rect).  option: TE_OPT_WINDOW_EXPR_ROUTE, as plan()
inline RegionPlan region_plan(int rows, int cols, int w, int n_red, int n_outer, int option, const region::Rect& dirty) {
  RegionPlan p;
  p.k = plan(rows, cols, w, n_red, n_outer, option);
  p.reach = p.k.m;
  p.out = region::grown(dirty, p.reach, p.reach, rows, cols);
  p.k.region = 1;
  p.k.oi0 = p.out.i0;
  p.k.oj0 = p.out.j0;
  p.k.oi1 = p.out.i1;
  p.k.oj1 = p.out.j1;
  p.k.tiles_i = (unsigned)((region::height(p.out) + kTI - 1) / kTI);
  p.k.tiles_j = (unsigned)((region::width(p.out) + kTJ - 1) / kTJ);
  p.k.tiles = (unsigned long long)p.k.tiles_i * p.k.tiles_j;  // (<= the whole map's, which plan() held against 2^31)
  return p;
}

// the cells of the map a workgroup stages (or, unstaged, may read through At): its tile with the halo, before the clamp
inline region::Rect staged(const Plan& k, unsigned tile) {
  int i0, j0;
  cell_of(k, tile, 0, &i0, &j0);
  return region::Rect{i0 - k.m, j0 - k.m, i0 - k.m + k.tile_rows, j0 - k.m + k.tile_cols};
}
// the cells of the input the call may read: out grown by m, clamped to the map
inline region::Rect window_reads(const RegionPlan& p, int rows, int cols) { return region::grown(p.out, p.reach, p.reach, rows, cols); }

}  // namespace wexpr
}  // namespace te
