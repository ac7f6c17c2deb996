// te_expr.hip -- the kernels of te_run_expression: a general MathExpressionFilter expression over the resident layers.
//   k_expr_map     one pass over the flat [batch][cols][rows] layers: every thread evaluates the program (te_expr.h) for the four
//                  cells of a 16-byte group.  The program arrives by value as a kernel argument, so the instruction stream is
//                  wave-uniform and the dispatch is a scalar branch per instruction; the operand stack lives in LDS as
//                  [slot][thread] (a runtime-indexed register array would go to scratch).  The top of the stack stays in
//                  registers: the shipped weighted sum touches LDS three times per group.
//   k_expr_rect    te_run_expression_region: the same evaluation on a rectangle of one map, no reductions.
//   k_expr_reduce  only for a program with reductions: evaluates every reduction argument per cell, folds a workgroup's
//                  kReduceSpan cells in a fixed order and writes one partial (double sum, float min / max, count) per block.
//   k_expr_finish  folds the partials of one (map, reduction) in a fixed order and writes the float32 result, which k_expr_map
//                  reads by the cell's map index.
// No float atomics, no waits between workgroups: the results are the same bits run after run.  In-place is legal (the output
// layer may be an operand): a thread reads its own four cells before it writes them, the reductions finish before the map pass.
#include "te_expr_launch.h"

namespace te {
namespace expr {
namespace {

constexpr int kThreads = 256;
typedef float float4a __attribute__((ext_vector_type(4)));
// four floats at any float boundary (k_expr_reduce: a map of an odd size starts at any 16-byte phase)
typedef float float4u __attribute__((ext_vector_type(4), aligned(4)));

struct LdsStack {
  float4a (*s)[kThreads];
  unsigned t;
  __device__ __forceinline__ void put(int k, const Vec<4>& v) { s[k][t] = float4a{v.v[0], v.v[1], v.v[2], v.v[3]}; }
  __device__ __forceinline__ Vec<4> get(int k) const {
    const float4a x = s[k][t];
    return Vec<4>{{x.x, x.y, x.z, x.w}};
  }
};

// the operands of the cells g .. g + 3 (flat index); `full`: all four exist, one 16-byte load; otherwise the first n do
template <class V4>
struct Source {
  const Args& a;
  size_t g;
  int n;
  const float* results;  // [batch][kMaxRed], nullptr in k_expr_reduce
  size_t map[4];         // of each cell (k_expr_map with reductions only)
  __device__ __forceinline__ Vec<4> layer(int slot) const {
    const float* p = a.in[slot] + g;
    if (n == 4) {
      const V4 x = *(const V4*)p;
      return Vec<4>{{x.x, x.y, x.z, x.w}};
    }
    Vec<4> r;
    for (int e = 0; e < 4; ++e) r.v[e] = e < n ? p[e] : 0.0f;
    return r;
  }
  __device__ __forceinline__ Vec<4> red(int k) const {
    Vec<4> r;
    for (int e = 0; e < 4; ++e) r.v[e] = results ? results[map[e] * kMaxRed + k] : 0.0f;
    return r;
  }
};

__global__ __launch_bounds__(kThreads) void k_expr_map(const Program p, const Args a, const float* results) {
  __shared__ float4a stk[kMaxStack - 1][kThreads];
  LdsStack st{stk, threadIdx.x};
  const size_t ngroups = (a.total + 3) >> 2;
  for (size_t q = (size_t)blockIdx.x * kThreads + threadIdx.x; q < ngroups; q += (size_t)gridDim.x * kThreads) {
    const size_t g = q << 2;
    const int n = a.total - g >= 4 ? 4 : (int)(a.total - g);
    Source<float4a> src{a, g, n, results, {0, 0, 0, 0}};
    if (results) {
      // a group may straddle two maps (an odd map size), or more on a map of fewer than four cells: per element
      const size_t m0 = g / a.cells, rem = g - m0 * a.cells;
      for (int e = 0; e < 4; ++e) {
        size_t m = a.cells >= 4 ? m0 + (rem + e >= a.cells ? 1 : 0) : (g + e) / a.cells;
        src.map[e] = e < n ? m : m0;  // (a cell behind the last one reads the result of a map that exists)
      }
    }
    const Vec<4> v = run<4>(p, 0, p.n_main, st, src);
    if (n == 4) {
      *(float4a*)(a.out + g) = float4a{v.v[0], v.v[1], v.v[2], v.v[3]};
    } else {
      for (int e = 0; e < 4; ++e)
        if (e < n) a.out[g + e] = v.v[e];
    }
  }
}

// te_run_expression_region: the cells [i0, i0 + h) x [j0, j0 + w) of one map (a.in / a.out point at the layers' first map,
// `base` is the map's offset in cells).  The rows of the rectangle run along the lanes, four consecutive rows of one column per
// thread -- the same run<4> as k_expr_map, element by element the same operations: the whole-map call's bits.  A column of the
// rectangle starts at any float boundary: 4-byte aligned loads and stores.  No reductions (the caller refuses them).
__global__ __launch_bounds__(kThreads) void k_expr_rect(const Program p, const Args a, size_t base, int rows, int i0, int j0, int h, int w) {
  __shared__ float4a stk[kMaxStack - 1][kThreads];
  LdsStack st{stk, threadIdx.x};
  const size_t per_col = ((size_t)h + 3) >> 2, ngroups = per_col * (size_t)w;
  for (size_t q = (size_t)blockIdx.x * kThreads + threadIdx.x; q < ngroups; q += (size_t)gridDim.x * kThreads) {
    const size_t col = q / per_col;
    const int di = (int)(q - col * per_col) << 2;
    const int n = h - di >= 4 ? 4 : h - di;
    const size_t g = base + ((size_t)j0 + col) * (size_t)rows + (size_t)(i0 + di);
    const Source<float4u> src{a, g, n, nullptr, {0, 0, 0, 0}};
    const Vec<4> v = run<4>(p, 0, p.n_main, st, src);
    if (n == 4) {
      *(float4u*)(a.out + g) = float4u{v.v[0], v.v[1], v.v[2], v.v[3]};
    } else {
      for (int e = 0; e < 4; ++e)
        if (e < n) a.out[g + e] = v.v[e];
    }
  }
}

// block (b, m): cells [b * kReduceSpan, ..) of map m, four per thread in order; parts[(m * n_red + r) * nblocks + b]
__global__ __launch_bounds__(kThreads) void k_expr_reduce(const Program p, const Args a, Partial* parts) {
  __shared__ float4a stk[kMaxStack - 1][kThreads];
  __shared__ Partial fold[kThreads];
  LdsStack st{stk, threadIdx.x};
  const size_t m = blockIdx.y, nblocks = gridDim.x;
  const size_t c = (size_t)blockIdx.x * kReduceSpan + 4 * (size_t)threadIdx.x;  // first cell of this thread, within the map
  const int n = c >= a.cells ? 0 : (a.cells - c >= 4 ? 4 : (int)(a.cells - c));
  const Source<float4u> src{a, m * a.cells + (n ? c : 0), n, nullptr, {0, 0, 0, 0}};
  for (int r = 0; r < p.n_red; ++r) {
    const int kind = p.red_kind[r];
    Partial q = partial_empty();
    if (n) {
      const Vec<4> v = run<4>(p, p.red_begin[r], p.red_end[r], st, src);
      for (int e = 0; e < 4; ++e)
        if (e < n) partial_add(q, kind, v.v[e]);
    }
    fold[threadIdx.x] = q;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {  // a fixed tree: the same order whatever the hardware schedules
      if ((int)threadIdx.x < s) {
        Partial x = fold[threadIdx.x];
        partial_merge(x, fold[threadIdx.x + s]);
        fold[threadIdx.x] = x;
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) parts[(m * p.n_red + r) * nblocks + blockIdx.x] = fold[0];
    __syncthreads();
  }
}

// block (r, m): thread t folds the partials t, t + kFinishThreads, .. in order, then the fixed tree
__global__ __launch_bounds__(kFinishThreads) void k_expr_finish(const Program p, const Partial* parts, size_t nblocks, size_t cells, float* results) {
  __shared__ Partial fold[kFinishThreads];
  const size_t r = blockIdx.x, m = blockIdx.y;
  const Partial* mine = parts + (m * p.n_red + r) * nblocks;
  Partial q = partial_empty();
  for (size_t b = threadIdx.x; b < nblocks; b += kFinishThreads) partial_merge(q, mine[b]);
  fold[threadIdx.x] = q;
  __syncthreads();
  for (int s = kFinishThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      Partial x = fold[threadIdx.x];
      partial_merge(x, fold[threadIdx.x + s]);
      fold[threadIdx.x] = x;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) results[m * kMaxRed + r] = partial_result(fold[0], p.red_kind[r], cells);
}

}  // namespace

hipError_t launch(const Program& p, const Args& a, size_t batch, void* scratch, hipStream_t stream) {
  const float* results = nullptr;
  if (p.n_red > 0) {
    const size_t nblocks = reduce_blocks(a.cells);
    Partial* parts = (Partial*)scratch;
    float* res = (float*)(parts + batch * (size_t)p.n_red * nblocks);
    hipLaunchKernelGGL(k_expr_reduce, dim3((unsigned)nblocks, (unsigned)batch), dim3(kThreads), 0, stream, p, a, parts);
    hipLaunchKernelGGL(k_expr_finish, dim3((unsigned)p.n_red, (unsigned)batch), dim3(kFinishThreads), 0, stream, p, (const Partial*)parts, nblocks, a.cells, res);
    results = res;
  }
  const size_t ngroups = (a.total + 3) >> 2;
  size_t blocks = (ngroups + kThreads - 1) / kThreads;
  if (blocks > 8192) blocks = 8192;  // (grid-stride beyond: 32 blocks per CU)
  hipLaunchKernelGGL(k_expr_map, dim3((unsigned)blocks), dim3(kThreads), 0, stream, p, a, results);
  return hipGetLastError();
}

hipError_t launch_rect(const Program& p, const Args& a, int rows, int cols, int map, int i0, int j0, int h, int w, hipStream_t stream) {
  // a rectangle of the map and a program without reductions: anything else is a caller's error, never a launch
  if (p.n_red > 0 || map < 0 || i0 < 0 || j0 < 0 || h <= 0 || w <= 0 || h > rows - i0 || w > cols - j0 || (size_t)rows * cols != a.cells ||
      ((size_t)map + 1) * a.cells > a.total)
    return hipErrorInvalidValue;
  const size_t ngroups = (((size_t)h + 3) >> 2) * (size_t)w;
  size_t blocks = (ngroups + kThreads - 1) / kThreads;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(k_expr_rect, dim3((unsigned)blocks), dim3(kThreads), 0, stream, p, a, (size_t)map * a.cells, rows, i0, j0, h, w);
  return hipGetLastError();
}

}  // namespace expr
}  // namespace te
