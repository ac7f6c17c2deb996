// te_components_launch.h -- the launcher of te_components.hip as te_components_api.hip sees it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "te_components_plan.h"

namespace te {
namespace components {

// the start cells of te_run_reachable as linear indices (col * rows + row), passed to the kernel by value
struct Starts {
  int n;
  uint32_t cell[kMaxStarts];
};

// One call's launch: `nmaps` maps of p.rows x p.cols cells (column-major, rows contiguous) behind `in` and `out`, which may be
// the same memory; scratch: p.scratch_bytes; counts: the four numbers of te_components_stats on the device.
struct Args {
  const float* in;
  float* out;
  void* scratch;
  unsigned long long* counts;
  int nmaps;
  int mode;
  float threshold;
  int connectivity;
};

// starts == NULL: te_run_components; else te_run_reachable (nmaps == 1)
hipError_t launch(const Plan& p, const Args& a, const Starts* starts, hipStream_t stream);

}  // namespace components
}  // namespace te
