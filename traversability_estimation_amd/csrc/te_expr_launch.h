// te_expr_launch.h -- the launchers of te_expr.hip as te_expr_api.hip sees them.
#pragma once
#include <hip/hip_runtime.h>

#include "te_expr.h"

namespace te {
namespace expr {

struct Args {
  const float* in[kMaxLayers];  // by the program's slot; any of them may be `out`
  float* out;
  size_t cells;  // of one map
  size_t total;  // batch * cells
};

// cells one workgroup of k_expr_reduce covers, and the partials one thread of k_expr_finish starts from
constexpr int kReduceSpan = 1024;
constexpr int kFinishThreads = 64;

inline size_t reduce_blocks(size_t cells) { return (cells + kReduceSpan - 1) / kReduceSpan; }
// bytes of the scratch a program with reductions needs: the partials [batch][n_red][blocks], then the results [batch][kMaxRed]
inline size_t scratch_bytes(const Program& p, size_t cells, size_t batch) {
  return batch * (size_t)p.n_red * reduce_blocks(cells) * sizeof(Partial) + batch * kMaxRed * sizeof(float);
}
// the launches of one evaluation, in order on `stream`; `scratch` (scratch_bytes, 8-byte aligned) only with reductions
hipError_t launch(const Program& p, const Args& a, size_t batch, void* scratch, hipStream_t stream);
// te_run_expression_region: the program on the cells [i0, i0 + h) x [j0, j0 + w) of map `map` (rows x cols cells, a.cells of
// them); no reductions, no scratch.  hipErrorInvalidValue: the rectangle is not one of the map, or the program has a reduction.
hipError_t launch_rect(const Program& p, const Args& a, int rows, int cols, int map, int i0, int j0, int h, int w, hipStream_t stream);

}  // namespace expr
}  // namespace te
