// te_distance_plan.h -- te_run_distance and te_run_distance_region as a plan: plain C++, no HIP, shared with the CPU test
// (tests/cpu/distance_plan_check.cpp).  The cap in cells, the rectangles of a call, the route of pass 2 and the launch geometry
// of both passes; the launcher (te_distance.hip) and the entry points (te_distance_api.hip) decide nothing of their own.
//
// Cap: cap2 = the largest integer k with (double)k * (res * res) <= max_distance * max_distance (the rounded product is
// monotone in k, so a bisection finds it without a division), R = floor(sqrt(cap2)): no seed farther than R cells along
// either axis can be within the cap.
//
// Rectangles (all clamped to the map; te_region_plan.h: grown).  A seed that changed inside `dirty` changes the output
// within R cells of it and nowhere else:
//   out   dirty grown by R                 the cells written
//   g     out grown by R along j           pass 1 computes the column distances there, pass 2 reads them (same rows as out)
//   in    g grown by R along i             the cells of the input pass 1 reads: no farther than 2 R from dirty
// The whole-map call is the same plan with dirty = the map.  g lives in scratch of its own size, columns of height(g).
//
// Pass 1: a wavefront owns seg_chunks * 64 consecutive rows of one column of g and scans them with a halo of R rows on
// either side; four wavefronts (columns) per workgroup.  seg_chunks grows with R so that the halo stays below half the work.
// Pass 2: a workgroup owns a tile of 64 rows x 64 columns of out, a lane a row of it.  The tiled route stages the tile's rows of
// g with R columns on either side in LDS (2 bytes per cell); the route of any reach reads g from memory.
//
// Route by plan (TE_OPT_DISTANCE_ROUTE = 0): tiled while it fits in kMaxLds and R <= kTiledMaxReach.  Measured
// (tools/distance_bench.py, profiles/distance_bench.json; DESIGN.md section 5 names the rows).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "te_distance.h"
#include "te_region_plan.h"

namespace te {
namespace distance {

constexpr int kMaxReach = 32767;
constexpr int kTI = 64, kTJ = 64, kWaves = 4, kThreads = kLanes * kWaves;
constexpr int kCellsPerLane = kTJ / kWaves;
// 64 KiB of the CU's 160 KiB: two workgroups stay resident at the largest halo, and the tiled route loses to the other one
// long before a larger tile would fit (see the route rows of profiles/distance_bench.json)
constexpr size_t kMaxLds = 64 * 1024;
constexpr int kTiledMaxReach = 64;
constexpr int kMaxSegChunks = 64;  // (a lane keeps the mask of one chunk of its wavefront's segment)
constexpr unsigned long long kMaxBlocks = 0x7fffffffull;

enum Route { kRouteTiled = 1, kRouteAny = 2 };

// false: max_distance is not finite and positive, or R would exceed kMaxReach.  res: finite and positive (te_set_geometry)
inline bool cap_of(double max_distance, double res, uint32_t* cap2, int* R) {
  if (!(max_distance > 0.0) || !isfinite(max_distance)) return false;
  const double q = max_distance * max_distance, r2 = res * res;
  const uint32_t limit = 1u << 30;  // cap2 >= 2^30 is R >= 32768
  if (!(q < INFINITY) || (double)limit * r2 <= q) return false;
  uint32_t lo = 0, hi = limit;  // k = lo satisfies the rule (0 <= q), k = hi does not
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if ((double)mid * r2 <= q)
      lo = mid;
    else
      hi = mid;
  }
  *cap2 = lo;
  int r = (int)sqrt((double)lo);
  while ((uint64_t)r * (uint64_t)r > lo) --r;
  while ((uint64_t)(r + 1) * (uint64_t)(r + 1) <= lo) ++r;
  *R = r;
  return true;
}

struct Plan {
  uint32_t cap2;
  int R;
  region::Rect out, g, in;
  int rows, cols;  // of the map
  int route;
  int lds_cols;      // columns of g a workgroup of the tiled route stages at most
  size_t lds_bytes;  // of the tiled route (0 on the other)
  size_t g_cells;    // cells of g per map
  // pass 1: workgroup b owns segment b % p1_segs of the columns g.j0 + (b / p1_segs) * kWaves + wave
  int seg_chunks;
  unsigned p1_segs;
  unsigned long long p1_blocks;
  // pass 2: workgroup b owns tile (b % tiles_i, b / tiles_i) of the grid over out
  unsigned tiles_i, tiles_j;
  unsigned long long p2_blocks;
  bool fits;  // both grids are launchable
};

inline int div_up(long long a, long long b) { return (int)((a + b - 1) / b); }

// option: TE_OPT_DISTANCE_ROUTE -- 0 by plan, 1 the tiled route wherever it fits, 2 the route of any reach always.
// `dirty` lies in the map (region::valid_rect); the whole-map call passes the map.
inline Plan plan(int rows, int cols, uint32_t cap2, int R, int option, const region::Rect& dirty) {
  Plan p;
  p.cap2 = cap2;
  p.R = R;
  p.rows = rows;
  p.cols = cols;
  p.out = region::grown(dirty, R, R, rows, cols);
  p.g = region::grown(p.out, 0, R, rows, cols);
  p.in = region::grown(p.g, R, 0, rows, cols);
  p.g_cells = region::cells(p.g);
  const long long gw = region::width(p.g), gh = region::height(p.g);
  const long long staged = (long long)kTJ + 2ll * R < gw ? (long long)kTJ + 2ll * R : gw;
  const unsigned long long lds = (unsigned long long)staged * kTI * sizeof(uint16_t);
  bool tiled = option != 2 && lds <= kMaxLds;
  if (option == 0 && R > kTiledMaxReach) tiled = false;
  p.route = tiled ? kRouteTiled : kRouteAny;
  p.lds_cols = tiled ? (int)staged : 0;
  p.lds_bytes = tiled ? (size_t)lds : 0;
  // the halo of a segment in chunks, as far as the map has rows for it
  const long long halo = R < rows ? R : rows, chunks = (gh + kLanes - 1) / kLanes;
  long long seg = 4 * ((halo + kLanes - 1) / kLanes);
  seg = seg < 4 ? 4 : seg;
  seg = seg > kMaxSegChunks ? kMaxSegChunks : seg;
  seg = seg > chunks ? chunks : seg;
  p.seg_chunks = (int)seg;
  p.p1_segs = (unsigned)((chunks + seg - 1) / seg);
  p.p1_blocks = (unsigned long long)p.p1_segs * (unsigned long long)((gw + kWaves - 1) / kWaves);
  p.tiles_i = (unsigned)div_up(region::height(p.out), kTI);
  p.tiles_j = (unsigned)div_up(region::width(p.out), kTJ);
  p.p2_blocks = (unsigned long long)p.tiles_i * p.tiles_j;
  p.fits = p.p1_blocks <= kMaxBlocks && p.p2_blocks <= kMaxBlocks;
  return p;
}

// Pass 1, wavefront `wave` of workgroup b: its column and the rows [*i0, *i1) of g it owns; false: none
TE_REGION_HD bool p1_unit(const Plan& p, unsigned long long b, int wave, int* i0, int* i1, int* j) {
  const long long col = (long long)p.g.j0 + (long long)(b / p.p1_segs) * kWaves + wave;
  const long long first = (long long)p.g.i0 + (long long)(b % p.p1_segs) * p.seg_chunks * kLanes;
  if (col >= p.g.j1 || first >= p.g.i1) return false;
  const long long end = first + (long long)p.seg_chunks * kLanes;
  *j = (int)col;
  *i0 = (int)first;
  *i1 = end < p.g.i1 ? (int)end : p.g.i1;
  return true;
}
// Pass 2, workgroup b: the first cell of its tile
TE_REGION_HD void p2_tile(const Plan& p, unsigned long long b, int* i0, int* j0) {
  *i0 = p.out.i0 + (int)(b % p.tiles_i) * kTI;
  *j0 = p.out.j0 + (int)(b / p.tiles_i) * kTJ;
}
// ... and the k-th cell (k < kCellsPerLane) of lane `lane` of wavefront `wave` in it; false: outside out
TE_REGION_HD bool p2_cell(const Plan& p, int i0, int j0, int wave, int lane, int k, int* i, int* j) {
  *i = i0 + lane;
  *j = j0 + wave + k * kWaves;
  return *i < p.out.i1 && *j < p.out.j1;
}
// the columns [*c0, *c1) of g the tile at column j0 reads (the tiled route stages exactly these)
TE_REGION_HD void p2_columns(const Plan& p, int j0, int* c0, int* c1) {
  const long long a = (long long)j0 - p.R, b = (long long)j0 + kTJ + p.R;
  *c0 = a < p.g.j0 ? p.g.j0 : (int)a;
  *c1 = b > p.g.j1 ? p.g.j1 : (int)b;
}

}  // namespace distance
}  // namespace te
