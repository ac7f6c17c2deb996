// te_pointwise_launch.h -- the launchers of te_pointwise.hip as te_pointwise_api.hip sees them.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace te {
namespace pointwise {

// gridMapFilters/ThresholdFilter in place on the n floats at p (any float boundary): lower -- v < t ? set_to : v, otherwise
// v > t ? set_to : v; a NaN stays.  n == 0 launches nothing.
hipError_t launch_threshold(float* p, size_t n, bool lower, float t, float set_to, hipStream_t stream);
// ... on the cells [i0, i0 + h) x [j0, j0 + w) of the one map of rows x cols cells at p.  hipErrorInvalidValue: the rectangle is
// not one of the map (never a launch).
hipError_t launch_threshold_rect(float* p, int rows, int cols, int i0, int j0, int h, int w, bool lower, float t, float set_to, hipStream_t stream);

}  // namespace pointwise
}  // namespace te
