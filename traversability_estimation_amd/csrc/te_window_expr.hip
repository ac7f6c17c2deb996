// te_window_expr.hip -- gridMapFilters/SlidingWindowMathExpressionFilter on the device (te_run_window_expression; the contract:
// include/travgpu.h; the plan: te_window_plan.h; the language, the evaluator and the folds over a window:
// te_expr.h).
//
// One kernel, one cell per lane, 32 x 8 cells per workgroup with the lanes of a wavefront along the contiguous axis i.  The
// program arrives by value as a kernel argument: the instruction stream is wave-uniform, the dispatch a scalar branch per
// instruction.  The operand stack below its top and the results of the reductions live in LDS as [slot][lane].  The tile
// with its halo of m cells is staged in LDS while the plan says it fits; otherwise At reads global memory.  Every read of the
// map goes through At, which checks the cell against the map first: a cell beyond the map is the padding, never a load.
//
//   direct     direct_cell: rule 3 gives the window, `mean` pads a clipped one with its own meanOfFinites, then
//              expr::window_reduce folds every inner reduction and after them every outer one, column by column.
//   separable  pass A: expr::window_column for every (cell row of the tile, column of the tile with its halo) and reduction,
//              into LDS as arrays; pass B: each cell merges the columns of its window in ascending order.  The same
//              functions in the same order as window_reduce: the same bits.  A workgroup that wg_separable() refuses
//              (`mean` with a clipped window) walks directly; the branch is uniform over the workgroup.
// A region call (te_run_window_expression_region, plan: te_region_plan.h) is the second instantiation of the kernel: the tiles
// start at the plan's origin and a lane owns a cell below the plan's end; staging, At and both routes are the same code.
// Built with -ffp-contract=off like every source of the library.
#include "te_window_expr_launch.h"

namespace te {
namespace wexpr {

namespace {

using expr::Partial;
using expr::Program;
using expr::Vec;

struct LdsStack {
  float (*s)[kThreads];
  unsigned t;
  __device__ __forceinline__ void put(int k, const Vec<1>& v) { s[k][t] = v.v[0]; }
  __device__ __forceinline__ Vec<1> get(int k) const { return Vec<1>{{s[k][t]}}; }
};

struct LdsRes {
  float (*r)[kThreads];
  unsigned t;
  __device__ __forceinline__ float get(int k) const { return r[k][t]; }
};

// the value of W at map coordinates: the padding beyond the map, else the staged tile or the layer itself
struct At {
  const float* __restrict__ in;    // the map
  const float* tile;               // nullptr: not staged
  int rows, cols, ia, ja, pitch;   // the tile holds rows [ia, ia + pitch) of columns [ja, ..)
  float pad;
  __device__ __forceinline__ float operator()(int row, int col) const {
    if (row < 0 || row >= rows || col < 0 || col >= cols) return pad;
    return tile ? tile[(col - ja) * pitch + (row - ia)] : in[(size_t)col * rows + row];
  }
};

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < INFINITY; }

// cell (i, j) of the map by the contract's own walk; 0 <= i < rows, 0 <= j < cols
__device__ float direct_cell(const Program& p, const Args& a, int m, LdsStack& st, LdsRes& res, At& at, int i, int j) {
  at.pad = __builtin_nanf("");
  const Extent e = extent(a.edge, m, a.rows, a.cols, i, j, finite_f(at(i, j)), a.compute_empty_cells != 0);
  if (!e.visited) return __builtin_nanf("");
  if (a.edge == kMean && e.clipped) at.pad = expr::window_mean_of_finites(at, e.blo, e.bhi, e.bclo, e.bchi);
  const int levels = p.n_outer > 0 ? 2 : 1;
#pragma unroll 1
  for (int level = 0; level < levels; ++level)
#pragma unroll 1
    for (int r = 0; r < p.n_red; ++r)
      if (p.red_level[r] == level) res.r[r][res.t] = expr::window_reduce(p, r, st, res, at, e.rlo, e.rhi, e.clo, e.chi);
  const expr::WindowSource<LdsRes> src{0.0f, &res};
  return expr::run<1>(p, 0, p.n_main, st, src).v[0];
}

// kRegion: a region call (te_region_plan.h) -- the tiles start at the plan's origin and own the cells below its end; a.in and
// a.out point at the one map.  Every read still goes through At and the staging's own check against the MAP.
template <bool kRegion>
__global__ __launch_bounds__(kThreads) void k_window_expr(const Program p, const Args a, const Plan pl) {
  extern __shared__ double lds_d[];
  char* lds = (char*)lds_d;
  const unsigned tid = threadIdx.x;
  LdsStack st{(float (*)[kThreads])lds, tid};
  LdsRes res{(float (*)[kThreads])(lds + (size_t)kStackSlots * kThreads * sizeof(float)), tid};
  float* T = pl.tile_in_lds ? (float*)(lds + pl.off_tile) : nullptr;

  const size_t mo = (size_t)blockIdx.y * a.rows * a.cols;
  const float* __restrict__ in = a.in + mo;
  float* __restrict__ out = a.out + mo;
  const int m = pl.m;
  int i, j;
  cell_of(pl.tiles_i, blockIdx.x, (int)tid, &i, &j);
  if (kRegion) {
    i += pl.oi0;
    j += pl.oj0;
  }
  const int ii = (int)tid % kTI;
  const int i0 = i - ii, j0 = j - (int)tid / kTI;
  At at{in, T, a.rows, a.cols, i0 - m, j0 - m, pl.tile_rows, __builtin_nanf("")};

  if (T) {
    const int n = pl.tile_rows * pl.tile_cols;
    for (int k = (int)tid; k < n; k += kThreads) {
      const int row = at.ia + k % pl.tile_rows, col = at.ja + k / pl.tile_rows;
      const bool inside = row >= 0 && row < a.rows && col >= 0 && col < a.cols;
      T[k] = inside ? in[(size_t)col * a.rows + row] : __builtin_nanf("");
    }
    __syncthreads();
  }
  const bool sep = pl.route == kRouteSeparable && wg_separable(a.edge, m, a.rows, a.cols, i0, j0);
  if (tid == 0) atomicAdd(&a.counts[sep ? 0 : 1], 1ull);
  const bool mine = kRegion ? i < pl.oi1 && j < pl.oj1 : i < a.rows && j < a.cols;
  if (!sep) {
    if (mine) out[(size_t)j * a.rows + i] = direct_cell(p, a, m, st, res, at, i, j);
    return;
  }

  // ---- pass A: the column partials of every (cell row, column of the tile with its halo), as arrays [reduction][column][row]
  const int n_items = kTI * pl.tile_cols, n_part = p.n_red * n_items;
  double* S = (double*)(lds + pl.off_part);
  float* MN = (float*)(S + n_part);
  float* MX = MN + n_part;
  uint32_t* CN = (uint32_t*)(MX + n_part);
  const bool clip = a.edge == kInside || a.edge == kCrop;  // W = B: a column beyond the map is no column of any window
#pragma unroll 1
  for (int item = (int)tid; item < n_items; item += kThreads) {
    const int row = i0 + item % kTI, col = j0 - m + item / kTI;
    if (row >= a.rows || (clip && (col < 0 || col >= a.cols))) continue;
    const int rlo = clip && row - m < 0 ? 0 : row - m, rhi = clip && row + m > a.rows - 1 ? a.rows - 1 : row + m;
#pragma unroll 1
    for (int r = 0; r < p.n_red; ++r) {
      const Partial q = expr::window_column(p, r, st, res, at, col, rlo, rhi);
      const int k = r * n_items + item;
      S[k] = q.sum;
      MN[k] = q.mn;
      MX[k] = q.mx;
      CN[k] = q.cnt;
    }
  }
  __syncthreads();
  if (!mine) return;

  // ---- pass B: the columns of the cell's window in ascending order
  const Extent e = extent(a.edge, m, a.rows, a.cols, i, j, finite_f(at(i, j)), a.compute_empty_cells != 0);
  float v = __builtin_nanf("");
  if (e.visited) {
    const uint64_t cells = (uint64_t)(e.rhi - e.rlo + 1) * (uint64_t)(e.chi - e.clo + 1);
#pragma unroll 1
    for (int r = 0; r < p.n_red; ++r) {
      Partial acc = expr::partial_empty();
#pragma unroll 1
      for (int col = e.clo; col <= e.chi; ++col) {
        const int k = r * n_items + (col - (j0 - m)) * kTI + ii;
        Partial q;
        q.sum = S[k];
        q.mn = MN[k];
        q.mx = MX[k];
        q.cnt = CN[k];
        q._pad = 0;
        expr::partial_merge(acc, q);
      }
      res.r[r][tid] = expr::partial_result(acc, p.red_kind[r], cells);
    }
    const expr::WindowSource<LdsRes> src{0.0f, &res};
    v = expr::run<1>(p, 0, p.n_main, st, src).v[0];
  }
  out[(size_t)j * a.rows + i] = v;
}

}  // namespace

hipError_t launch(const Program& prog, const Args& a, const Plan& p, hipStream_t stream) {
  if (a.nmaps <= 0) return hipSuccess;
  if (!p.fits || p.lds_bytes > kMaxLds) return hipErrorInvalidValue;
  if (p.region) {
    // the origin and the end lie in the map and the tiles cover exactly [oi0, oi1) x [oj0, oj1): anything else is no plan
    if (a.nmaps != 1 || p.oi0 < 0 || p.oj0 < 0 || p.oi1 > a.rows || p.oj1 > a.cols || p.oi1 <= p.oi0 || p.oj1 <= p.oj0 ||
        p.tiles_i != (unsigned)((p.oi1 - p.oi0 + kTI - 1) / kTI) || p.tiles != (unsigned long long)p.tiles_i * (unsigned)((p.oj1 - p.oj0 + kTJ - 1) / kTJ))
      return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_window_expr<true>, dim3((unsigned)p.tiles, 1u), dim3(kThreads), p.lds_bytes, stream, prog, a, p);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_window_expr<false>, dim3((unsigned)p.tiles, (unsigned)a.nmaps), dim3(kThreads), p.lds_bytes, stream, prog, a, p);
  return hipGetLastError();
}

}  // namespace wexpr
}  // namespace te
