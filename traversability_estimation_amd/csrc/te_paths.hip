// te_paths.hip -- batched TraversabilityMap::checkFootprintPath for circular footprints
// (traversability_estimation/src/TraversabilityMap.cpp:320-342 -> checkCircularFootprintPath :344-462) on the
// resident traversability_footprint layer.  With the layer complete, isTraversable(center, ...) takes its memo
// branch for every centre (:672-677: value = layer, traversable = value != 0), so a path is a walk over
// LineIterator cells (every fourth, nSkip :396) with a running mean and a length-weighted mean over the
// segments.  One thread per path: planners check thousands of short candidate paths per cycle.
// footprint/check_robot_inclination (:114, robot_footprint_parameter.yaml:10): with the layer robot_slope given,
// checkInclination (:748-762) runs before every pose / segment (:366-370, :390-394); the same test batched on its
// own is k_check_inclination (the polygonal path check uses it, :526-528, :553-557).
// Not covered (reference defaults): publishPolygons, compute_untraversable_polygon.
#include "te_geom.h"
#include "te_internal.h"
#include "te_path_walk.h"

namespace te {

namespace {

__global__ __launch_bounds__(256) void k_check_inclination(Geo g, const float* __restrict__ robot_slope, int n,
                                                           const double* __restrict__ start_end_xy,
                                                           unsigned char* __restrict__ ok, int* __restrict__ status) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const double* q = start_end_xy + 4 * (size_t)k;
  bool outside;
  ok[k] = inclination_ok(g, robot_slope, q[0], q[1], q[2], q[3], outside) ? 1 : 0;
  status[k] = outside ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_check_circular_paths(Geo g, const float* __restrict__ footprint, double fp_default,
                                                              const float* __restrict__ robot_slope, int n_paths, const int* __restrict__ pose_offset,
                                                              const double* __restrict__ pose_xy,
                                                              unsigned char* __restrict__ is_safe,
                                                              double* __restrict__ traversability, int* __restrict__ status) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_paths) return;
  const int p0 = pose_offset[k], n = pose_offset[k + 1] - p0;
  unsigned char safe;
  double out;
  int st;
  check_circular_path(g, robot_slope, fp_default, n, pose_xy + 2 * (size_t)p0,
                      [&](int i, int j) { return (double)footprint[(size_t)j * g.rows + i]; }, safe, out, st);
  is_safe[k] = safe;
  traversability[k] = out;
  status[k] = st;
}

}  // namespace

hipError_t launch_check_circular_paths(const Geo& g, const float* footprint, double fp_default, const float* robot_slope,
                                       int n_paths, const int* pose_offset, const double* pose_xy, unsigned char* is_safe,
                                       double* traversability, int* status, hipStream_t stream) {
  if (n_paths <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_check_circular_paths, dim3((unsigned)((n_paths + 255) / 256)), dim3(256), 0, stream, g, footprint,
                     fp_default, robot_slope, n_paths, pose_offset, pose_xy, is_safe, traversability, status);
  return hipGetLastError();
}

hipError_t launch_check_inclination(const Geo& g, const float* robot_slope, int n, const double* start_end_xy,
                                    unsigned char* ok, int* status, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_check_inclination, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, g, robot_slope, n,
                     start_end_xy, ok, status);
  return hipGetLastError();
}

}  // namespace te
