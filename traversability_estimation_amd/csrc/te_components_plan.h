// te_components_plan.h -- te_run_components / te_run_reachable as a plan: plain C++, no HIP, shared with the CPU test
// (tests/cpu/components_check.cpp).  The tile edges, the grids of the four launches, the scratch and the refusals; the launcher
// (te_components.hip) and the entry points (te_components_api.hip) decide nothing of their own.
//
// One route.  A tile is ti rows x tj columns (64 x 64 on the device: a wavefront's ballot is one column of it); tile (a, b)
// owns the cells [a * ti, (a + 1) * ti) x [b * tj, (b + 1) * tj) of the map.  A seam is the border between two tiles: the
// column seams are the first columns of the tile columns 1 .. tiles_j - 1 (every row of the map), the row seams the first rows of
// the tile rows 1 .. tiles_i - 1 (every column).  Seam cell u of a map: the column seams first, rows fastest.
// Launches, whatever the map holds: tile pass, seam pass (none on a map of one tile), flatten + count, the starts
// (te_run_reachable), write.  Scratch: a label and a count of 32 bits each per cell of the call, 8 bytes per cell.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "te_region_plan.h"

namespace te {
namespace components {

constexpr int kTI = 64, kTJ = 64, kWaves = 4, kThreads = 64 * kWaves;
constexpr int kMaxStarts = 256;  // TE_REACHABLE_MAX_STARTS
constexpr unsigned long long kMaxBlocks = 0x7fffffffull;
constexpr unsigned kWriteBlocksMax = 4096;  // the write pass walks the map with a stride: four atomics per workgroup for the counts
constexpr size_t kScratchPerCell = 2 * sizeof(uint32_t);

struct Plan {
  int rows, cols;  // of the map
  int ti, tj;      // tile edges
  unsigned tiles_i, tiles_j;
  unsigned long long cells;          // of a map
  unsigned long long tile_blocks;    // tile pass: workgroup b owns tile (b % tiles_i, b / tiles_i)
  unsigned long long col_seam_cells, seam_cells;  // per map
  unsigned long long seam_blocks;    // seam pass: kThreads seam cells per workgroup
  unsigned long long flat_blocks;    // flatten + count: kThreads cells per workgroup
  unsigned write_blocks;             // write: cell x, x + write_blocks * kThreads, ... per thread
  size_t scratch_bytes;              // of the call: labels of every map, then counts of every map
  bool fits;                         // fewer than 2^31 cells per map and every grid launchable
};

inline unsigned long long div_up_ull(unsigned long long a, unsigned long long b) { return (a + b - 1) / b; }

// rows, cols >= 1, nmaps >= 1; 1 <= ti <= 64 and 1 <= tj <= 64 (the CPU test forces small ones)
inline Plan plan(int rows, int cols, int nmaps, int ti = kTI, int tj = kTJ) {
  Plan p;
  p.rows = rows, p.cols = cols, p.ti = ti, p.tj = tj;
  p.tiles_i = (unsigned)div_up_ull((unsigned long long)rows, (unsigned long long)ti);
  p.tiles_j = (unsigned)div_up_ull((unsigned long long)cols, (unsigned long long)tj);
  p.cells = (unsigned long long)rows * (unsigned long long)cols;
  p.tile_blocks = (unsigned long long)p.tiles_i * p.tiles_j;
  p.col_seam_cells = (unsigned long long)(p.tiles_j - 1) * (unsigned long long)rows;
  p.seam_cells = p.col_seam_cells + (unsigned long long)(p.tiles_i - 1) * (unsigned long long)cols;
  p.seam_blocks = div_up_ull(p.seam_cells, kThreads);
  p.flat_blocks = div_up_ull(p.cells, kThreads);
  p.write_blocks = (unsigned)(p.flat_blocks < kWriteBlocksMax ? p.flat_blocks : kWriteBlocksMax);
  p.scratch_bytes = (size_t)p.cells * (size_t)nmaps * kScratchPerCell;
  p.fits = p.cells < (1ull << 31) && p.tile_blocks <= kMaxBlocks && p.flat_blocks <= kMaxBlocks && nmaps <= 65535 &&
           p.cells * (unsigned long long)nmaps <= (~(size_t)0) / kScratchPerCell;
  return p;
}

// tile pass, workgroup b: the first cell of its tile
TE_REGION_HD void tile_origin(const Plan& p, unsigned long long b, int* i0, int* j0) {
  *i0 = (int)(b % p.tiles_i) * p.ti;
  *j0 = (int)(b / p.tiles_i) * p.tj;
}
// seam pass, seam cell u < p.seam_cells: its cell, and whether it lies on a column seam (else a row seam)
TE_REGION_HD void seam_cell(const Plan& p, unsigned long long u, bool* col_seam, int* i, int* j) {
  if (u < p.col_seam_cells) {
    *col_seam = true;
    *i = (int)(u % (unsigned long long)p.rows);
    *j = ((int)(u / (unsigned long long)p.rows) + 1) * p.tj;
  } else {
    const unsigned long long v = u - p.col_seam_cells;
    *col_seam = false;
    *j = (int)(v % (unsigned long long)p.cols);
    *i = ((int)(v / (unsigned long long)p.cols) + 1) * p.ti;
  }
}

}  // namespace components
}  // namespace te
