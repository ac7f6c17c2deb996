// te_median_launch.h -- the launchers of te_median.hip as te_median_api.hip sees them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "te_median_plan.h"
#include "te_region_plan.h"

namespace te {
namespace median {

// One call's launches, `nmaps` maps of rows x cols cells (column-major, rows contiguous) behind each pointer.
struct Args {
  const float* in;  // never the memory `out` points to
  float* out;
  uint8_t* mask;    // out: shouldFill per cell, kept for te_download_fill_mask
  uint8_t* tmp[2];  // scratch of the mask passes, nmaps * cells bytes each
  // the general route's scratch, for one map at a time: a count per 256 cells (any_blocks(cells) + 1 entries, the last one
  // the total) and the list of cells to select for (at most `cells` entries)
  unsigned* any_counts;
  unsigned* any_list;
  int rows, cols, nmaps;
  int r_fill;
  int r_exist;  // -1: finite cells keep their values (filter_existing_values off, or an existing radius of 0 cells)
  int iterations;
};

constexpr int kAnyBlock = 256;
inline size_t any_blocks(size_t cells) { return (cells + kAnyBlock - 1) / kAnyBlock; }

// the launches of one call in order on `stream`: the mask passes, then the route the plan names
hipError_t launch(const Args& a, const Plan& p, hipStream_t stream);
// te_run_median_fill_region: the same on the rectangles of `p`, for ONE map -- in, out, mask and tmp point at that map's cells
// (tmp: rows * cols bytes each), any_counts holds p.any_blocks + 1 entries and any_list as many as p.out has cells
hipError_t launch_region(const Args& a, const RegionPlan& p, hipStream_t stream);

}  // namespace median
}  // namespace te
