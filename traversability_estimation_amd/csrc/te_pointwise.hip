// te_pointwise.hip -- the kernels of te_run_threshold(_region): gridMapFilters/ThresholdFilter in place on a layer.
//   k_threshold       one streaming pass over a flat run of floats (whole maps are contiguous): the floats before the first
//                     16-byte boundary and behind the last one go one per thread, everything between as 16-byte loads and stores.
//   k_threshold_rect  a rectangle of one map: four consecutive rows of one column per thread, as k_expr_rect (te_expr.hip) walks
//                     it; a column of the rectangle starts at any float boundary, so its groups are 4-byte aligned 16-byte
//                     accesses.
// The comparison is te_expr.h's threshold_lower / threshold_upper, the function the two fused opcodes of the expression
// evaluator call: te_run_layer_expression_thresholds writes these bits.  Every thread reads a cell before it writes it and no
// other thread touches that cell: in place is safe.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "te_expr.h"
#include "te_pointwise_launch.h"

namespace te {
namespace pointwise {
namespace {

constexpr int kThreads = 256;
constexpr size_t kMaxBlocks = 8192;  // (grid-stride beyond: 32 blocks per CU, as k_expr_map)
typedef float float4a __attribute__((ext_vector_type(4)));
typedef float float4u __attribute__((ext_vector_type(4), aligned(4)));

template <bool LOWER>
__device__ __forceinline__ float apply(float v, float t, float s) {
  return LOWER ? expr::threshold_lower(v, t, s) : expr::threshold_upper(v, t, s);
}

// p[0 .. n): head floats up to the first 16-byte boundary (head <= 3, head <= n), then ngroups aligned groups, then the rest
template <bool LOWER>
__global__ __launch_bounds__(kThreads) void k_threshold(float* p, size_t n, size_t head, size_t ngroups, float t, float s) {
  const size_t tid = (size_t)blockIdx.x * kThreads + threadIdx.x, stride = (size_t)gridDim.x * kThreads;
  float4a* const body = (float4a*)(p + head);
  for (size_t q = tid; q < ngroups; q += stride) {
    float4a x = body[q];
    x.x = apply<LOWER>(x.x, t, s);
    x.y = apply<LOWER>(x.y, t, s);
    x.z = apply<LOWER>(x.z, t, s);
    x.w = apply<LOWER>(x.w, t, s);
    body[q] = x;
  }
  // at most 3 + 3 single floats: the first threads of the grid take one each
  const size_t tail0 = head + 4 * ngroups, n_single = head + (n - tail0);
  if (tid < n_single) {
    const size_t i = tid < head ? tid : tail0 + (tid - head);
    p[i] = apply<LOWER>(p[i], t, s);
  }
}

template <bool LOWER>
__global__ __launch_bounds__(kThreads) void k_threshold_rect(float* p, int rows, int i0, int j0, int h, int w, float t, float s) {
  const size_t per_col = ((size_t)h + 3) >> 2, ngroups = per_col * (size_t)w;
  for (size_t q = (size_t)blockIdx.x * kThreads + threadIdx.x; q < ngroups; q += (size_t)gridDim.x * kThreads) {
    const size_t col = q / per_col;
    const int di = (int)(q - col * per_col) << 2;
    const int n = h - di >= 4 ? 4 : h - di;
    float* const g = p + ((size_t)j0 + col) * (size_t)rows + (size_t)(i0 + di);
    if (n == 4) {
      float4u x = *(const float4u*)g;
      x.x = apply<LOWER>(x.x, t, s);
      x.y = apply<LOWER>(x.y, t, s);
      x.z = apply<LOWER>(x.z, t, s);
      x.w = apply<LOWER>(x.w, t, s);
      *(float4u*)g = x;
    } else {
      for (int e = 0; e < n; ++e) g[e] = apply<LOWER>(g[e], t, s);
    }
  }
}

unsigned grid_for(size_t work) {
  size_t blocks = (work + kThreads - 1) / kThreads;
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  return (unsigned)(blocks ? blocks : 1);
}

}  // namespace

hipError_t launch_threshold(float* p, size_t n, bool lower, float t, float set_to, hipStream_t stream) {
  if (!n) return hipSuccess;
  if (!p || ((uintptr_t)p & 3u)) return hipErrorInvalidValue;
  size_t head = ((16 - ((uintptr_t)p & 15u)) & 15u) >> 2;
  if (head > n) head = n;
  const size_t ngroups = (n - head) >> 2;
  const unsigned grid = grid_for(ngroups > 6 ? ngroups : 6);  // (the single floats need the first six threads)
  if (lower)
    hipLaunchKernelGGL(k_threshold<true>, dim3(grid), dim3(kThreads), 0, stream, p, n, head, ngroups, t, set_to);
  else
    hipLaunchKernelGGL(k_threshold<false>, dim3(grid), dim3(kThreads), 0, stream, p, n, head, ngroups, t, set_to);
  return hipGetLastError();
}

hipError_t launch_threshold_rect(float* p, int rows, int cols, int i0, int j0, int h, int w, bool lower, float t, float set_to, hipStream_t stream) {
  if (!p || rows <= 0 || cols <= 0 || i0 < 0 || j0 < 0 || h <= 0 || w <= 0 || h > rows - i0 || w > cols - j0) return hipErrorInvalidValue;
  const unsigned grid = grid_for((((size_t)h + 3) >> 2) * (size_t)w);
  if (lower)
    hipLaunchKernelGGL(k_threshold_rect<true>, dim3(grid), dim3(kThreads), 0, stream, p, rows, i0, j0, h, w, t, set_to);
  else
    hipLaunchKernelGGL(k_threshold_rect<false>, dim3(grid), dim3(kThreads), 0, stream, p, rows, i0, j0, h, w, t, set_to);
  return hipGetLastError();
}

}  // namespace pointwise
}  // namespace te
