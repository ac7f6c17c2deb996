// te_radius_launch.h -- the launcher of te_radius.hip as te_radius_api.hip sees it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "te_internal.h"
#include "te_radius_plan.h"
#include "te_region_plan.h"

namespace te {
namespace radius {

// the window of a call on the device (te_radius_plan.h: Shape): tab = hw[0 .. R], then the sorted ties as (di, dj) pairs
struct Window {
  const int32_t* tab;
  double r2;  // radius * radius, as CircleIterator computes it (the ties)
  int R, hw0, reach, n_ties;
};

// One call's launch, `nmaps` maps of rows x cols cells (column-major, rows contiguous) behind each pointer.
struct Args {
  const float* in;  // never the memory `out` points to
  float* out;
  unsigned long long* counts;  // [2]: workgroups the sliding kernel settled / workgroups the gather settled (added to)
  int nmaps;
  int op;
};

hipError_t launch(const Geo& g, const Window& w, const Args& a, const Plan& p, hipStream_t stream);
// te_run_radius_filter_region: the centres of p.out of ONE map -- in and out point at that map's cells (a.nmaps is not read)
hipError_t launch_region(const Geo& g, const Window& w, const Args& a, const RegionPlan& p, hipStream_t stream);

}  // namespace radius
}  // namespace te
