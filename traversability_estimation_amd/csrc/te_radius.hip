// te_radius.hip -- gridMapFilters/MeanInRadiusFilter and MinInRadiusFilter on the device (te_run_radius_filter; the contract:
// include/travgpu.h; the plan and the predicate: te_radius_plan.h).
//
// The window is the CircleIterator disc of te_disc_table.h: runs hw[0 .. R] and tie offsets, the ties decided per centre
// with the reference's double arithmetic (tie_inside, as te_filter_any.hip has it).  A cell outside the map is no cell and
// every load is bounds-checked.  One centre per lane, the lanes of a wavefront along the contiguous axis i.
//
//   k_radius_gather  the contract's walk, literally: row offset ascending, column offset ascending, the ties merged in at
//                    their place (a tie lies outside the run of its row: before it for dj < 0, after it for dj > 0).  Mean: a
//                    double sum and a count of the finite values in that order.  Min: the ordered minimum of them.
//   k_radius_slide   64 x 16 centres per workgroup walk the source columns within R of theirs.  Min: range-minimum tables of
//                    each column segment, two LDS reads per run.  Mean: prefix sums in double and prefix counts of each
//                    column segment, a run is a difference of two prefixes; taken only by a workgroup for whose cells
//                    order_free() holds (decided over every cell it can read, ties included, before it stages anything),
//                    otherwise the workgroup runs gather_cell for its centres.  The branch is uniform over the workgroup.
// Both kernels take the rectangle of centres they own (region::Rect): the whole map, or the output rectangle of
// te_run_radius_filter_region (te_region_plan.h), whose workgroup tiles start at its corner.  What a centre READS is bounded by
// the map alone.
// Built with -ffp-contract=off like every source of the library.
#include "te_radius_launch.h"

namespace te {
namespace radius {

namespace {

__device__ __forceinline__ bool finite_f(float v) { return __builtin_isfinite(v); }

// the smaller of two values, NaN skipped, -0.0 below +0.0 (the contract's order; v_min_f32 leaves the zeros' order open)
__device__ __forceinline__ float min_ord(float a, float b) {
  if (!(b == b)) return a;
  if (!(a == a)) return b;
  if (a < b) return a;
  if (b < a) return b;
  return __builtin_signbit(a) ? a : b;
}
__device__ __forceinline__ float sanitize(float v) { return finite_f(v) ? v : __builtin_nanf(""); }

// CircleIterator::isInside for one offset, with the reference's own double arithmetic (te_filter_any.hip)
__device__ __forceinline__ bool tie_inside(const Geo& g, double r2, int i, int j, int di, int dj) {
  const double cx = g.ax + g.res * (double)(-i);
  const double cy = g.ay + g.res * (double)(-j);
  const double x = g.ax + g.res * (double)(-(i + di));
  const double y = g.ay + g.res * (double)(-(j + dj));
  const double dx = x - cx, dy = y - cy;
  return dx * dx + dy * dy <= r2;
}

__device__ __forceinline__ int tie_di(const Window& w, int t) { return w.tab[w.R + 1 + 2 * t]; }
__device__ __forceinline__ int tie_dj(const Window& w, int t) { return w.tab[w.R + 2 + 2 * t]; }

struct Acc {
  double sum;
  int n;
  float mn;
};
template <int OP>
__device__ __forceinline__ void take(Acc& a, float v) {
  if (OP == kMean) {
    if (finite_f(v)) {
      a.sum += (double)v;
      ++a.n;
    }
  } else {
    a.mn = min_ord(a.mn, sanitize(v));
  }
}
template <int OP>
__device__ __forceinline__ float result(const Acc& a) {
  if (OP == kMean) return a.n > 0 ? (float)(a.sum / (double)a.n) : __builtin_nanf("");
  return a.mn;
}
// tie t of centre (i, j), if it is a cell of the map and inside this centre's circle
template <int OP>
__device__ __forceinline__ void take_tie(Acc& a, const Geo& g, const Window& w, const float* __restrict__ in, int i, int j, int t) {
  const int di = tie_di(w, t), dj = tie_dj(w, t);
  const int ii = i + di, jj = j + dj;
  if (ii < 0 || ii >= g.rows || jj < 0 || jj >= g.cols || !tie_inside(g, w.r2, i, j, di, dj)) return;
  take<OP>(a, in[(size_t)jj * g.rows + ii]);
}

// the window of centre (i, j) of the map at `in`, in the contract's order; 0 <= i < rows, 0 <= j < cols
template <int OP>
__device__ float gather_cell(const Geo& g, const Window& w, const float* __restrict__ in, int i, int j) {
  Acc a = {0.0, 0, __builtin_nanf("")};
  const int dlo = -w.reach < -i ? -i : -w.reach;
  const int dhi = w.reach > g.rows - 1 - i ? g.rows - 1 - i : w.reach;
  int t = 0;
#pragma unroll 1
  for (int di = dlo; di <= dhi; ++di) {
    while (t < w.n_ties && tie_di(w, t) < di) ++t;
    const int ad = di < 0 ? -di : di;
    const int h = ad <= w.R ? w.tab[ad] : -1;
    const int ii = i + di;  // in [0, rows) by dlo, dhi
    while (t < w.n_ties && tie_di(w, t) == di && tie_dj(w, t) < 0) take_tie<OP>(a, g, w, in, i, j, t++);
    if (h >= 0) {
      const int lo = -h < -j ? -j : -h;
      const int hi = h > g.cols - 1 - j ? g.cols - 1 - j : h;
#pragma unroll 1
      for (int dj = lo; dj <= hi; ++dj) take<OP>(a, in[(size_t)(j + dj) * g.rows + ii]);
    }
    while (t < w.n_ties && tie_di(w, t) == di) take_tie<OP>(a, g, w, in, i, j, t++);
  }
  return result<OP>(a);
}

template <int OP>
__global__ __launch_bounds__(kThreads) void k_radius_gather(Geo g, Window w, region::Rect own, const float* __restrict__ in, float* __restrict__ out,
                                                           unsigned long long* __restrict__ counts) {
  const size_t mo = (size_t)blockIdx.z * g.rows * g.cols;
  const int i = own.i0 + blockIdx.x * kTX + threadIdx.x;
  if (threadIdx.x == 0 && threadIdx.y == 0) atomicAdd(&counts[1], 1ull);
  if (i >= own.i1) return;  // (own lies in the map)
  for (long long j = (long long)own.j0 + (long long)blockIdx.y * kWaves + threadIdx.y; j < own.j1; j += (long long)gridDim.y * kWaves)
    out[mo + (size_t)j * g.rows + i] = gather_cell<OP>(g, w, in + mo, i, (int)j);
}

__device__ __forceinline__ int ilog2(int v) { return 31 - __clz(v); }

constexpr int kCPT = kTY / kWaves;  // centres per lane

// `seg`: rows of a staged segment (te_radius_plan.h: segment_len); levels: of the Min tables; log2n: of the predicate
template <int OP>
__global__ __launch_bounds__(kThreads) void k_radius_slide(Geo g, Window w, region::Rect own, int seg, int levels, int log2n, const float* __restrict__ in_all,
                                                          float* __restrict__ out_all, unsigned long long* __restrict__ counts) {
  extern __shared__ double lds_d[];
  const size_t mo = (size_t)blockIdx.z * g.rows * g.cols;
  const float* __restrict__ in = in_all + mo;
  float* __restrict__ out = out_all + mo;
  const int tid = threadIdx.y * kTX + threadIdx.x;
  const int i0 = own.i0 + blockIdx.x * kTX, j0 = own.j0 + blockIdx.y * kTY;  // (own lies in the map: i0 < rows, j0 < cols)
  const int i = i0 + threadIdx.x;
  const int H = w.hw0;
  const int sa = i0 - H < 0 ? 0 : i0 - H;
  const int sb = i0 + kTX + H > g.rows ? g.rows : i0 + kTX + H;
  const int n = sb - sa;  // 1 <= n <= seg
  const int jlo = j0 - w.R < 0 ? 0 : j0 - w.R;
  const int jhi = w.R < 0 ? jlo - 1 : (j0 + kTY - 1 + w.R >= g.cols ? g.cols - 1 : j0 + kTY - 1 + w.R);  // (no run: no column)

  if (OP == kMin) {
    float* MN = (float*)lds_d;  // [levels][seg]
    float mn[kCPT];
#pragma unroll
    for (int c = 0; c < kCPT; ++c) mn[c] = __builtin_nanf("");
#pragma unroll 1
    for (int jp = jlo; jp <= jhi; ++jp) {
      __syncthreads();
      const float* col = in + (size_t)jp * g.rows + sa;
      for (int t = tid; t < n; t += kThreads) MN[t] = sanitize(col[t]);
      __syncthreads();
      for (int k = 1; k < levels; ++k) {
        const int half = 1 << (k - 1);
        for (int t = tid; t + (1 << k) <= n; t += kThreads) MN[k * seg + t] = min_ord(MN[(k - 1) * seg + t], MN[(k - 1) * seg + t + half]);
        __syncthreads();
      }
#pragma unroll
      for (int c = 0; c < kCPT; ++c) {
        const int j = j0 + threadIdx.y + c * kWaves;
        const int b = j > jp ? j - jp : jp - j;
        if (i >= own.i1 || j >= own.j1 || b > w.R) continue;
        const int h = w.tab[b];
        if (h < 0) continue;
        const int lo = (i - h < sa ? sa : i - h) - sa, hi = (i + h >= sb ? sb - 1 : i + h) - sa;  // lo <= i - sa <= hi
        const int k = ilog2(hi - lo + 1);  // k < levels: hi - lo + 1 <= min(2 H + 1, n)
        mn[c] = min_ord(mn[c], min_ord(MN[k * seg + lo], MN[k * seg + hi - (1 << k) + 1]));
      }
    }
#pragma unroll
    for (int c = 0; c < kCPT; ++c) {
      const int j = j0 + threadIdx.y + c * kWaves;
      if (i >= own.i1 || j >= own.j1) continue;
      Acc a = {0.0, 0, mn[c]};
      for (int t = 0; t < w.n_ties; ++t) take_tie<kMin>(a, g, w, in, i, j, t);
      out[(size_t)j * g.rows + i] = a.mn;
    }
    if (tid == 0) atomicAdd(&counts[0], 1ull);
    return;
  }

  // ---- Mean ----
  double* P = lds_d;                    // [seg + 1] prefix sums of the finite cells of the segment
  double* S = P + (seg + 1);            // [2][kThreads] the scan of the chunk sums
  int* C = (int*)(S + 2 * kThreads);    // [seg + 1] prefix counts
  int* K = C + (seg + 1);               // [2][kThreads]
  int* ex = K + 2 * kThreads;           // emax, emin

  // the predicate over every cell a centre of this workgroup can read: the runs and the ties, `reach` cells around the centres
  if (tid == 0) {
    ex[0] = -1000;
    ex[1] = 1000;
  }
  __syncthreads();
  {
    const int pa = i0 - w.reach < 0 ? 0 : i0 - w.reach;
    const int pb = i0 + kTX + w.reach > g.rows ? g.rows : i0 + kTX + w.reach;
    const int qa = j0 - w.reach < 0 ? 0 : j0 - w.reach;
    const int qb = j0 + kTY + w.reach > g.cols ? g.cols : j0 + kTY + w.reach;
    const int pn = pb - pa;
    int emax = -1000, emin = 1000;
    for (int jp = qa + (int)threadIdx.y; jp < qb; jp += kWaves) {
      const float* col = in + (size_t)jp * g.rows + pa;
      for (int t = threadIdx.x; t < pn; t += kTX) {
        const float v = col[t];
        const uint32_t bits = __float_as_uint(v);
        if (finite_f(v) && (bits & 0x7fffffffu) != 0u) {
          const int e = float_exponent(bits);
          emax = e > emax ? e : emax;
          emin = e < emin ? e : emin;
        }
      }
    }
    if (emax >= emin) {
      atomicMax(&ex[0], emax);
      atomicMin(&ex[1], emin);
    }
  }
  __syncthreads();
  const bool exact = order_free(ex[0], ex[1], log2n);
  if (tid == 0) atomicAdd(&counts[exact ? 0 : 1], 1ull);
  if (!exact) {
#pragma unroll 1
    for (int c = 0; c < kCPT; ++c) {
      const int j = j0 + threadIdx.y + c * kWaves;
      if (i < own.i1 && j < own.j1) out[(size_t)j * g.rows + i] = gather_cell<kMean>(g, w, in, i, j);
    }
    return;
  }

  double sum[kCPT];
  int cnt[kCPT];
#pragma unroll
  for (int c = 0; c < kCPT; ++c) sum[c] = 0.0, cnt[c] = 0;
  const int L = (n + kThreads - 1) / kThreads;  // cells per lane of the scan
  const int nch = (n + L - 1) / L;              // lanes that hold a chunk, <= kThreads
  const int c0 = tid * L, c1 = c0 + L < n ? c0 + L : n;
#pragma unroll 1
  for (int jp = jlo; jp <= jhi; ++jp) {
    const float* col = in + (size_t)jp * g.rows + sa;
    double s = 0.0;
    int k = 0;
    for (int t = c0; t < c1; ++t) {
      const float v = col[t];
      if (finite_f(v)) s += (double)v, ++k;
    }
    __syncthreads();  // the reads of the column before are done
    S[tid] = s;
    K[tid] = k;
    __syncthreads();
    int src = 0;
    for (int off = 1; off < nch; off <<= 1) {  // inclusive scan of the chunk sums (exact in any order under the predicate)
      const int dst = src ^ 1;
      double x = S[src * kThreads + tid];
      int y = K[src * kThreads + tid];
      if (tid >= off) x += S[src * kThreads + tid - off], y += K[src * kThreads + tid - off];
      S[dst * kThreads + tid] = x;
      K[dst * kThreads + tid] = y;
      __syncthreads();
      src = dst;
    }
    if (tid < nch) {
      double x = tid > 0 ? S[src * kThreads + tid - 1] : 0.0;
      int y = tid > 0 ? K[src * kThreads + tid - 1] : 0;
      if (tid == 0) P[0] = 0.0, C[0] = 0;
      for (int t = c0; t < c1; ++t) {
        const float v = col[t];
        if (finite_f(v)) x += (double)v, ++y;
        P[t + 1] = x;
        C[t + 1] = y;
      }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kCPT; ++c) {
      const int j = j0 + threadIdx.y + c * kWaves;
      const int b = j > jp ? j - jp : jp - j;
      if (i >= own.i1 || j >= own.j1 || b > w.R) continue;
      const int h = w.tab[b];
      if (h < 0) continue;
      const int lo = (i - h < sa ? sa : i - h) - sa, hi = (i + h >= sb ? sb - 1 : i + h) - sa;  // 0 <= lo <= hi < n
      sum[c] += P[hi + 1] - P[lo];
      cnt[c] += C[hi + 1] - C[lo];
    }
  }
#pragma unroll
  for (int c = 0; c < kCPT; ++c) {
    const int j = j0 + threadIdx.y + c * kWaves;
    if (i >= own.i1 || j >= own.j1) continue;
    Acc a = {sum[c], cnt[c], 0.0f};
    for (int t = 0; t < w.n_ties; ++t) take_tie<kMean>(a, g, w, in, i, j, t);
    out[(size_t)j * g.rows + i] = result<kMean>(a);
  }
}

}  // namespace

static hipError_t launch_on(const Geo& g, const Window& w, const Args& a, const Plan& p, const region::Rect& own, unsigned nmaps, hipStream_t stream) {
  const dim3 grid(p.grid_x, p.grid_y, nmaps), block(kTX, kWaves);
  if (p.route == kRouteSlide) {
    if (a.op == kMean)
      hipLaunchKernelGGL(k_radius_slide<kMean>, grid, block, p.lds_bytes, stream, g, w, own, p.seg, p.levels, p.log2n, a.in, a.out, a.counts);
    else
      hipLaunchKernelGGL(k_radius_slide<kMin>, grid, block, p.lds_bytes, stream, g, w, own, p.seg, p.levels, p.log2n, a.in, a.out, a.counts);
  } else {
    if (a.op == kMean)
      hipLaunchKernelGGL(k_radius_gather<kMean>, grid, block, 0, stream, g, w, own, a.in, a.out, a.counts);
    else
      hipLaunchKernelGGL(k_radius_gather<kMin>, grid, block, 0, stream, g, w, own, a.in, a.out, a.counts);
  }
  return hipGetLastError();
}

hipError_t launch(const Geo& g, const Window& w, const Args& a, const Plan& p, hipStream_t stream) {
  if (a.nmaps <= 0) return hipSuccess;
  const region::Rect whole = {0, 0, g.rows, g.cols};
  return launch_on(g, w, a, p, whole, (unsigned)a.nmaps, stream);
}

hipError_t launch_region(const Geo& g, const Window& w, const Args& a, const RegionPlan& p, hipStream_t stream) {
  const region::Rect& o = p.out;
  if (o.i0 < 0 || o.j0 < 0 || o.i0 >= o.i1 || o.j0 >= o.j1 || o.i1 > g.rows || o.j1 > g.cols) return hipErrorInvalidValue;
  return launch_on(g, w, a, p.k, o, 1u, stream);
}

}  // namespace radius
}  // namespace te
