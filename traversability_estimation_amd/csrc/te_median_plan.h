// te_median_plan.h -- te_run_median_fill as a plan: plain C++, no HIP, shared with the CPU test (tests/cpu/median_plan_check.cpp).
// The window radius in cells, the tile the hot kernel stages, its LDS bytes, and which kernel a (rows, cols, r) takes.  The
// launcher (te_median_api.hip) decides nothing of its own, and every index the kernels form is bounded by what is here.
//
// Radius in cells: grid_map_filters' MedianFillFilter computes `(size_t)(radius / resolution)` -- a double division,
// truncated, with no rounding fix: 0.15 / 0.05 is 2.9999999999999996 and gives 2.  (Restated from memory, like the rest of the
// filter: include/travgpu.h.)
//
// Tile route (k_median_tile): a workgroup of 256 lanes owns kTileRows x kTileCols = 64 x 16 cells (rows are contiguous in
// memory) and stages them with a halo of r cells on every side as 32-bit keys, followed by its list of cells to select
// for (one uint16 per tile cell).  Budget: kLdsBudget = 20 KiB per workgroup, so that eight workgroups -- 32 wavefronts,
// a compute unit's full complement -- fit the 160 KiB of LDS and LDS never limits occupancy; that admits r <= 15, where the
// staged rectangle is 4.2 x the tile.  Above it the halo is most of what a workgroup loads, and the general kernel
// (k_median_any, one wavefront per selected cell, the window read from global memory) takes over.  It serves any radius.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

namespace te {
namespace median {

constexpr int kTileRows = 64, kTileCols = 16, kTileThreads = 256;
constexpr int kTileCells = kTileRows * kTileCols;
constexpr size_t kLdsBudget = 20 * 1024;
constexpr int kMaxTileBlocks = 0x7fffffff;  // (a grid's x extent)

enum Route { kRouteTile = 1, kRouteAny = 2 };

// `(size_t)(radius / resolution)`; radius finite and >= 0, resolution finite and > 0 (the callers have checked).  Windows
// are clamped to the map, so a radius beyond the map's longer side selects over the whole map: the count is cut there, which
// keeps it an int whatever the quotient is.
inline int radius_cells(double radius, double resolution, int rows, int cols) {
  const double q = radius / resolution;
  const int cap = rows > cols ? rows : cols;
  if (!(q < (double)cap)) return cap;
  return (int)(size_t)q;
}
// (the quotient alone: what Python's int(radius / res) is compared with)
inline unsigned long long radius_cells_unclamped(double radius, double resolution) { return (unsigned long long)(size_t)(radius / resolution); }

// dynamic LDS of a k_median_tile workgroup at halo r: the staged keys, then the list
inline size_t tile_lds_bytes(int r) {
  const size_t w = (size_t)kTileRows + 2 * (size_t)r, h = (size_t)kTileCols + 2 * (size_t)r;
  return w * h * sizeof(uint32_t) + (size_t)kTileCells * sizeof(uint16_t);
}
// (the kernel's 16 vote counts are static LDS on top of what the launch passes)
constexpr size_t kTileStaticLds = 64;
inline bool tile_fits(int r) { return r >= 0 && r <= 4096 && tile_lds_bytes(r) + kTileStaticLds <= kLdsBudget; }

struct Plan {
  int r;              // the halo: the larger of the radii in use
  int route;          // kRouteTile / kRouteAny
  int tiles_x, tiles_y;  // tiles along the rows / the columns (both routes: the tile grid is also how a map is described)
  size_t lds_bytes;   // of the tile kernel (0 on the general route)
  size_t blocks;      // tile route: workgroups of the launch = tiles_x * tiles_y * nmaps
};

// option: TE_OPT_MEDIAN_ROUTE -- 0 by plan, 1 the tile kernel wherever its window fits, 2 the general kernel always.  By plan
// the tile kernel runs wherever it fits, so 0 and 1 agree today; 1 stays the way to ask for it by name.
inline Plan plan(int rows, int cols, int nmaps, int r, int option) {
  Plan p;
  p.r = r;
  p.tiles_x = (rows + kTileRows - 1) / kTileRows;
  p.tiles_y = (cols + kTileCols - 1) / kTileCols;
  p.blocks = (size_t)p.tiles_x * (size_t)p.tiles_y * (size_t)nmaps;
  const bool tile = option != 2 && tile_fits(r) && p.blocks <= (size_t)kMaxTileBlocks;
  p.route = tile ? kRouteTile : kRouteAny;
  p.lds_bytes = tile ? tile_lds_bytes(r) : 0;
  return p;
}

}  // namespace median
}  // namespace te
