// te_distance_launch.h -- the launcher of te_distance.hip as te_distance_api.hip sees it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "te_distance_plan.h"

namespace te {
namespace distance {

// One call's launch: `nmaps` maps of p.rows x p.cols cells (column-major, rows contiguous) behind `in` and `out`, which may be
// the same memory; g: nmaps * p.g_cells cells of scratch.
struct Args {
  const float* in;
  float* out;
  uint16_t* g;
  int nmaps;
  int mode;
  float threshold;
  double res;
  float beyond;  // (float)max_distance
};

enum Passes { kPass1 = 1, kPass2 = 2, kBothPasses = 3 };

// counts (may be NULL): the workgroups of pass 2 launched on the tiled route and on the route of any reach
hipError_t launch(const Plan& p, const Args& a, int passes, hipStream_t stream, unsigned long long counts[2]);

}  // namespace distance
}  // namespace te
