// te_window_expr_launch.h -- the launcher of te_window_expr.hip as te_window_expr_api.hip sees it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "te_expr.h"
#include "te_window_plan.h"

namespace te {
namespace wexpr {

// One call's launch, `nmaps` maps of rows x cols cells (column-major, rows contiguous) behind each pointer.
struct Args {
  const float* in;  // never the memory `out` points to
  float* out;
  unsigned long long* counts;  // [2]: workgroups the separable route settled / workgroups the direct walk settled (added to)
  int rows, cols, nmaps;
  int edge;                  // Edge
  int compute_empty_cells;
};

hipError_t launch(const expr::Program& prog, const Args& a, const Plan& p, hipStream_t stream);

}  // namespace wexpr
}  // namespace te
