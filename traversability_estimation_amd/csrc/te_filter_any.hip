// te_filter_any.hip -- the filters at any radius: normals / slope / roughness and both step passes for a disc marked
// Disc::any (above 32 cells or with more than 32 tie offsets under TE_OPT_FILTER_ANY_RADIUS = 1; every disc under 2).
//
// The disc comes from its device table (te_disc_table.h, uploaded by rebuild_tables): hw[0 .. R] as int32, then the tie
// offsets as (di, dj) int32 pairs.  Nothing here depends on kMaxRadiusCells, kMaxTies or the slab's guard rows: every load
// is bounds-checked and a cell outside the map is "no cell", as load_tile stages it.  One cell per lane, the lanes of a
// wavefront along the contiguous axis i.
//
//   k_fa_step_height  StepFilter pass 1 (StepFilter.cpp:112-144).  A block of 64 x 16 centres walks the source columns
//                     j' within R of its columns; each column segment [i0 - hw(0), i0 + 63 + hw(0)] is staged once into
//                     LDS as a sparse table of range max and range min (log2 levels), and every centre row j reads the run
//                     of |j - j'| as two LDS reads per table: O(R) per cell.  max and min are exact and NaN-skipping
//                     (fminf / fmaxf), so the result is bit-identical to k_step_height.
//   k_fa_step_score   StepFilter pass 2 (:147-178): the same walk over step_height with a range max (stepMax starting
//                     at 0.0) and a prefix count of the cells above the critical value and of the valid cells.
//   k_fa_step_exact   both passes as plain gathers from global memory (O(R^2) per cell), for a segment whose tables do
//                     not fit in 64 KiB of LDS (a disc of more than about 360 cells on a map that tall).
//   k_fa_normals      normals + slope + roughness (+ the combine), and RoughnessFilter with the layers' normals, from
//                     prefix moments of the same column segments: O(R) per cell; the cells whose scores it cannot decide
//                     safely (near a clip, ill-conditioned) are left to k_fa_exact.
//   k_fa_exact        the same outputs from the generic kernels' gather (accumulate_disc: run by run, the same order and
//                     arithmetic) from global memory, O(R^2) per cell: the fix-up pass behind k_fa_normals, every cell
//                     under TE_OPT_NORMALS_RANK_RULE or when the prefix sums outgrow 64 KiB of LDS.
// Built with -ffp-contract=off like every source of the library: tie_inside keeps the reference's un-fused arithmetic.
#include "te_cell.h"
#include "te_internal.h"

namespace te {

namespace {

constexpr int TX = 64;   // centres along i: one wavefront
constexpr int BY = 4;    // wavefronts along j
constexpr int TYB = 16;  // centres along j per block of the step kernels
constexpr int CPT = TYB / BY;
constexpr size_t kMaxLds = 64 * 1024;

__device__ __forceinline__ float sanitize(float v) { return __builtin_isfinite(v) ? v : __builtin_nanf(""); }

// the disc's run half-width of column offset +-b and its tie t, from the fixed arrays or from the device table
__device__ __forceinline__ int disc_hw(const Disc& d, int b) { return d.any ? d.tab[b] : d.hw[b]; }
__device__ __forceinline__ void disc_tie(const Disc& d, int t, int& di, int& dj) {
  if (d.any) {
    di = d.tab[d.R + 1 + 2 * t];
    dj = d.tab[d.R + 2 + 2 * t];
  } else {
    di = d.tie_di[t];
    dj = d.tie_dj[t];
  }
}

// CircleIterator::isInside for one offset, with the reference's own double arithmetic (te_kernels.hip)
__device__ __forceinline__ bool tie_inside(const Geo& g, double r2, int i, int j, int di, int dj) {
  const double cx = g.ax + g.res * (double)(-i);
  const double cy = g.ay + g.res * (double)(-j);
  const double x = g.ax + g.res * (double)(-(i + di));
  const double y = g.ay + g.res * (double)(-(j + dj));
  const double dx = x - cx, dy = y - cy;
  return dx * dx + dy * dy <= r2;
}

__device__ __forceinline__ int ilog2(int v) { return 31 - __clz(v); }

__device__ __forceinline__ float step_score(float smax, int ncells, bool valid, double crit, int ncrit) {
  if (!valid) return __builtin_nanf("");
  const double sm = (double)smax;
  const double a1 = (double)ncells / (double)ncrit * sm;
  const double step = sm < a1 ? sm : a1;  // StepFilter.cpp:170
  return step < crit ? (float)(1.0 - step / crit) : 0.0f;
}

// the column segment a block stages: rows [a, b) of the map around its 64 centres
struct Segment {
  int a, b, levels;
};
__device__ __forceinline__ Segment block_segment(const Geo& g, const Disc& d, int i0) {
  Segment s;
  const int H = d.R >= 0 ? disc_hw(d, 0) : 0;
  s.a = i0 - H < 0 ? 0 : i0 - H;
  s.b = i0 + TX + H > g.rows ? g.rows : i0 + TX + H;
  const int wmax = 2 * H + 1 < s.b - s.a ? 2 * H + 1 : s.b - s.a;
  s.levels = ilog2(wmax > 0 ? wmax : 1) + 1;
  return s;
}

// range reads over rows [lo, hi] of the staged segment (lo <= hi): two per table
__device__ __forceinline__ void range_reads(const float* T, int stride, int lo, int hi, float& v0, float& v1) {
  const int k = ilog2(hi - lo + 1);
  v0 = T[k * stride + lo];
  v1 = T[k * stride + hi - (1 << k) + 1];
}

// level 0 of the tables from column jp of `layer` (the map's base), then the log2 levels
template <bool MIN>
__device__ __forceinline__ void build_tables(float* MX, float* MN, int stride, const float* __restrict__ layer, const Geo& g, int jp,
                                             const Segment& s) {
  const int tid = threadIdx.y * TX + threadIdx.x;
  const int n = s.b - s.a;
  const float* col = layer + (size_t)jp * g.rows + s.a;
  for (int t = tid; t < n; t += TX * BY) {
    const float v = sanitize(col[t]);
    MX[t] = v;
    if (MIN) MN[t] = v;
  }
  __syncthreads();
  for (int k = 1; k < s.levels; ++k) {
    const int half = 1 << (k - 1);
    for (int t = tid; t + (1 << k) <= n; t += TX * BY) {
      MX[k * stride + t] = fmaxf(MX[(k - 1) * stride + t], MX[(k - 1) * stride + t + half]);
      if (MIN) MN[k * stride + t] = fminf(MN[(k - 1) * stride + t], MN[(k - 1) * stride + t + half]);
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------
// StepFilter pass 1
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TX* BY) void k_fa_step_height(Geo g, Disc d, int stride, const float* __restrict__ elev, float* __restrict__ sh,
                                                           Region rg) {
  extern __shared__ float lds[];
  const int map = rg.map >= 0 ? rg.map : blockIdx.z;
  const size_t mo = (size_t)map * g.rows * g.cols;
  const int i0 = rg.i0 + blockIdx.x * TX, j0 = rg.j0 + blockIdx.y * TYB;
  const Segment s = block_segment(g, d, i0);
  float* MX = lds;
  float* MN = lds + (size_t)s.levels * stride;
  const int i = i0 + threadIdx.x;
  float mx[CPT], mn[CPT];
  bool live[CPT];
#pragma unroll
  for (int c = 0; c < CPT; ++c) {
    const int j = j0 + threadIdx.y + c * BY;
    live[c] = i < rg.i1 && j < rg.j1;
    const float z0 = live[c] ? sanitize(elev[mo + (size_t)j * g.rows + i]) : __builtin_nanf("");
    live[c] = live[c] && z0 == z0;  // StepFilter.cpp:113 only cells with a valid elevation
    mx[c] = mn[c] = z0;
  }
  const int jlo = j0 - d.R < 0 ? 0 : j0 - d.R;
  const int jhi = j0 + TYB - 1 + d.R >= g.cols ? g.cols - 1 : j0 + TYB - 1 + d.R;
#pragma unroll 1
  for (int jp = jlo; jp <= jhi; ++jp) {
    __syncthreads();
    build_tables<true>(MX, MN, stride, elev + mo, g, jp, s);
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      const int j = j0 + threadIdx.y + c * BY;
      const int b = j > jp ? j - jp : jp - j;
      if (!live[c] || b > d.R) continue;
      const int h = disc_hw(d, b);
      if (h < 0) continue;
      const int lo = (i - h < s.a ? s.a : i - h) - s.a, hi = (i + h >= s.b ? s.b - 1 : i + h) - s.a;
      float a0, a1;
      range_reads(MX, stride, lo, hi, a0, a1);
      mx[c] = fmaxf(mx[c], fmaxf(a0, a1));  // fminf/fmaxf ignore NaN == the isValid() skip, :126
      range_reads(MN, stride, lo, hi, a0, a1);
      mn[c] = fminf(mn[c], fminf(a0, a1));
    }
  }
#pragma unroll
  for (int c = 0; c < CPT; ++c) {
    const int j = j0 + threadIdx.y + c * BY;
    if (i >= rg.i1 || j >= rg.j1) continue;
    if (live[c]) {
      for (int t = 0; t < d.n_ties; ++t) {
        int di, dj;
        disc_tie(d, t, di, dj);
        const int ii = i + di, jj = j + dj;
        if (ii < 0 || ii >= g.rows || jj < 0 || jj >= g.cols || !tie_inside(g, d.r2, i, j, di, dj)) continue;
        const float z = sanitize(elev[mo + (size_t)jj * g.rows + ii]);
        mn[c] = fminf(mn[c], z);
        mx[c] = fmaxf(mx[c], z);
      }
    }
    sh[mo + (size_t)j * g.rows + i] = live[c] ? (float)((double)mx[c] - (double)mn[c]) : __builtin_nanf("");  // :143
  }
}

// ------------------------------------------------------------------------------------------------
// StepFilter pass 2
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TX* BY) void k_fa_step_score(Geo g, Disc d, int stride, double crit, int ncrit, const float* __restrict__ sh,
                                                          float* __restrict__ out, Region rg) {
  extern __shared__ float lds[];
  __shared__ int wsum[BY];
  __shared__ int carry;
  const int map = rg.map >= 0 ? rg.map : blockIdx.z;
  const size_t mo = (size_t)map * g.rows * g.cols;
  const int i0 = rg.i0 + blockIdx.x * TX, j0 = rg.j0 + blockIdx.y * TYB;
  const Segment s = block_segment(g, d, i0);
  float* MX = lds;
  int* P = (int*)(lds + (size_t)s.levels * stride);  // [0 .. n]: prefix counts, (cells > crit) | (valid cells) << 16
  const int tid = threadIdx.y * TX + threadIdx.x, lane = threadIdx.x;
  const int n = s.b - s.a;
  const int i = i0 + threadIdx.x;
  float smax[CPT];
  int ncells[CPT];
  bool valid[CPT];
#pragma unroll
  for (int c = 0; c < CPT; ++c) {
    smax[c] = 0.0f;  // stepMax starts at 0.0, :149
    ncells[c] = 0;
    valid[c] = false;
  }
  const int jlo = j0 - d.R < 0 ? 0 : j0 - d.R;
  const int jhi = j0 + TYB - 1 + d.R >= g.cols ? g.cols - 1 : j0 + TYB - 1 + d.R;
#pragma unroll 1
  for (int jp = jlo; jp <= jhi; ++jp) {
    __syncthreads();
    build_tables<false>(MX, nullptr, stride, sh + mo, g, jp, s);
    // prefix counts of the staged column: a block scan, 256 rows at a time
    if (tid == 0) {
      carry = 0;
      P[0] = 0;
    }
    __syncthreads();
    for (int base = 0; base < n; base += TX * BY) {
      const int t = base + tid;
      int x = 0;
      if (t < n) {
        const float v = MX[t];
        x = (((double)v > crit) ? 1 : 0) | ((v == v) ? 1 << 16 : 0);  // (NaN compares false)
      }
#pragma unroll
      for (int off = 1; off < TX; off <<= 1) {
        const int y = __shfl_up(x, off);
        if (lane >= off) x += y;
      }
      if (lane == TX - 1) wsum[threadIdx.y] = x;
      __syncthreads();
      int add = carry;
      for (int w = 0; w < (int)threadIdx.y; ++w) add += wsum[w];
      if (t < n) P[t + 1] = x + add;
      __syncthreads();
      if (tid == TX * BY - 1) carry = x + add;
      __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      const int j = j0 + threadIdx.y + c * BY;
      const int b = j > jp ? j - jp : jp - j;
      if (i >= rg.i1 || j >= rg.j1 || b > d.R) continue;
      const int h = disc_hw(d, b);
      if (h < 0) continue;
      const int lo = (i - h < s.a ? s.a : i - h) - s.a, hi = (i + h >= s.b ? s.b - 1 : i + h) - s.a;
      float a0, a1;
      range_reads(MX, stride, lo, hi, a0, a1);
      smax[c] = fmaxf(smax[c], fmaxf(a0, a1));
      const int cnt = P[hi + 1] - P[lo];  // (both fields non-negative: no borrow)
      ncells[c] += cnt & 0xffff;
      valid[c] = valid[c] || (cnt >> 16) != 0;
    }
  }
#pragma unroll
  for (int c = 0; c < CPT; ++c) {
    const int j = j0 + threadIdx.y + c * BY;
    if (i >= rg.i1 || j >= rg.j1) continue;
    for (int t = 0; t < d.n_ties; ++t) {
      int di, dj;
      disc_tie(d, t, di, dj);
      const int ii = i + di, jj = j + dj;
      if (ii < 0 || ii >= g.rows || jj < 0 || jj >= g.cols || !tie_inside(g, d.r2, i, j, di, dj)) continue;
      const float v = sanitize(sh[mo + (size_t)jj * g.rows + ii]);
      valid[c] = valid[c] || (v == v);
      smax[c] = fmaxf(smax[c], v);
      ncells[c] += ((double)v > crit) ? 1 : 0;
    }
    out[mo + (size_t)j * g.rows + i] = step_score(smax[c], ncells[c], valid[c], crit, ncrit);
  }
}

// both step passes as plain gathers: the segments' tables do not fit in LDS
template <bool SCORE>
__global__ __launch_bounds__(TX* BY) void k_fa_step_exact(Geo g, Disc d, double crit, int ncrit, const float* __restrict__ in,
                                                          float* __restrict__ out, Region rg) {
  const int map = rg.map >= 0 ? rg.map : blockIdx.z;
  const size_t mo = (size_t)map * g.rows * g.cols;
  const int i = rg.i0 + blockIdx.x * TX + threadIdx.x, j = rg.j0 + blockIdx.y * BY + threadIdx.y;
  if (i >= rg.i1 || j >= rg.j1) return;
  const float* lay = in + mo;
  const float z0 = sanitize(lay[(size_t)j * g.rows + i]);
  if (!SCORE && !(z0 == z0)) {
    out[mo + (size_t)j * g.rows + i] = __builtin_nanf("");
    return;
  }
  float mx = SCORE ? 0.0f : z0, mn = z0;
  int ncells = 0;
  bool valid = false;
  auto take = [&](float v) {
    mx = fmaxf(mx, v);
    if (SCORE) {
      valid = valid || (v == v);
      ncells += ((double)v > crit) ? 1 : 0;
    } else {
      mn = fminf(mn, v);
    }
  };
  for (int dj = -d.R; dj <= d.R; ++dj) {
    const int jj = j + dj;
    if (jj < 0 || jj >= g.cols) continue;
    const int h = disc_hw(d, dj < 0 ? -dj : dj);
    const int lo = i - h < 0 ? 0 : i - h, hi = i + h >= g.rows ? g.rows - 1 : i + h;
    const float* row = lay + (size_t)jj * g.rows;
    for (int ii = lo; ii <= hi; ++ii) take(sanitize(row[ii]));
  }
  for (int t = 0; t < d.n_ties; ++t) {
    int di, dj;
    disc_tie(d, t, di, dj);
    const int ii = i + di, jj = j + dj;
    if (ii < 0 || ii >= g.rows || jj < 0 || jj >= g.cols || !tie_inside(g, d.r2, i, j, di, dj)) continue;
    take(sanitize(lay[(size_t)jj * g.rows + ii]));
  }
  out[mo + (size_t)j * g.rows + i] = SCORE ? step_score(mx, ncells, valid, crit, ncrit) : (float)((double)mx - (double)mn);
}

// ------------------------------------------------------------------------------------------------
// Normals + slope + roughness: the generic gather from global memory
// ------------------------------------------------------------------------------------------------
// Mom with 64-bit integer moments (the sum of dj^2 over a disc grows as R^4: int overflows from about 230 cells)
struct MomL {
  long long n, si, sj, sii, sij, sjj;
  double sz, siz, sjz, szz;
};

// accumulate_disc (te_kernels.hip) from the map's layer: run by run, the same order and arithmetic.  A cell outside the
// map adds exactly nothing there (NaN in the tile: +0.0 to sums that are never -0.0), so the runs are clipped to the map.
__device__ __forceinline__ void fa_gather(MomL& m, const Geo& g, const Disc& d, const float* __restrict__ lay, int i, int j, double z0) {
  m.n = m.si = m.sj = m.sii = m.sij = m.sjj = 0;
  m.sz = m.siz = m.sjz = m.szz = 0.0;
  for (int dj = -d.R; dj <= d.R; ++dj) {
    const int jj = j + dj;
    if (jj < 0 || jj >= g.cols) continue;
    const int hw = disc_hw(d, dj < 0 ? -dj : dj);
    const int lo = i - hw < 0 ? -i : -hw, hi = i + hw >= g.rows ? g.rows - 1 - i : hw;
    const float* row = lay + (size_t)jj * g.rows + i;
    long long rn = 0, rsi = 0, rsii = 0;
    double rsz = 0.0, rsiz = 0.0, rszz = 0.0;
#pragma unroll 4
    for (int di = lo; di <= hi; ++di) {
      const float z = row[di];
      const bool v = __builtin_isfinite(z);
      const double dz = v ? (double)z - z0 : 0.0;
      const int w = v ? 1 : 0;
      const int wdi = v ? di : 0;
      rn += w;
      rsi += wdi;
      rsii += (long long)wdi * di;
      rsz += dz;
      rsiz = fma((double)di, dz, rsiz);
      rszz = fma(dz, dz, rszz);
    }
    m.n += rn;
    m.si += rsi;
    m.sj += dj * rn;
    m.sii += rsii;
    m.sij += dj * rsi;
    m.sjj += (long long)dj * dj * rn;
    m.sz += rsz;
    m.siz += rsiz;
    m.sjz = fma((double)dj, rsz, m.sjz);
    m.szz += rszz;
  }
  for (int t = 0; t < d.n_ties; ++t) {  // mom_add
    int di, dj;
    disc_tie(d, t, di, dj);
    const int ii = i + di, jj = j + dj;
    if (ii < 0 || ii >= g.rows || jj < 0 || jj >= g.cols || !tie_inside(g, d.r2, i, j, di, dj)) continue;
    const float z = lay[(size_t)jj * g.rows + ii];
    if (!__builtin_isfinite(z)) continue;
    const double dz = (double)z - z0;
    m.n += 1;
    m.si += di;
    m.sj += dj;
    m.sii += (long long)di * di;
    m.sij += (long long)di * dj;
    m.sjj += (long long)dj * dj;
    m.sz += dz;
    m.siz = fma((double)di, dz, m.siz);
    m.sjz = fma((double)dj, dz, m.sjz);
    m.szz = fma(dz, dz, m.szz);
  }
}

// covariance (te_cell.h) from the 64-bit moments: the same arithmetic
__device__ __forceinline__ void fa_covariance(const MomL& m, double res, double c[6]) {
  const double n = (double)m.n;
  const double inv_n2 = 1.0 / (n * n);
  const double cii = (double)(m.n * m.sii - m.si * m.si);
  const double cij = (double)(m.n * m.sij - m.si * m.sj);
  const double cjj = (double)(m.n * m.sjj - m.sj * m.sj);
  const double ciz = fma(n, m.siz, -(double)m.si * m.sz);
  const double cjz = fma(n, m.sjz, -(double)m.sj * m.sz);
  const double czz = fma(n, m.szz, -m.sz * m.sz);
  const double r2 = res * res;
  c[0] = r2 * cii * inv_n2;
  c[1] = r2 * cij * inv_n2;
  c[2] = -res * ciz * inv_n2;
  c[3] = r2 * cjj * inv_n2;
  c[4] = -res * cjz * inv_n2;
  c[5] = czz * inv_n2;
}

// smallest_eigvec and normal_from_cov (te_cell.h), the same arithmetic inlined: the shared copy is a call whose array
// arguments live in scratch memory
__device__ __forceinline__ void fa_eigvec(const double c[6], double nrm[3], double& lambda1) {
  double a00 = c[0], a01 = c[1], a02 = c[2], a11 = c[3], a12 = c[4], a22 = c[5];
  double v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;
#pragma unroll 1
  for (int sweep = 0; sweep < 32; ++sweep) {
    const double off = fabs(a01) + fabs(a02) + fabs(a12);
    const double dia = fabs(a00) + fabs(a11) + fabs(a22);
    if (off == 0.0 || (sweep > 3 && dia + 100.0 * off == dia)) break;
    jacobi_rot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
    jacobi_rot(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
    jacobi_rot(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
  }
  double w0 = a00, w1 = a11, w2 = a22;
  double x0 = v00, x1 = v10, x2 = v20;
  double y0 = v01, y1 = v11, y2 = v21;
  double z0 = v02, z1 = v12, z2 = v22;
  if (w1 < w0 && w1 <= w2) {
    double t;
    t = w0; w0 = w1; w1 = t;
    t = x0; x0 = y0; y0 = t; t = x1; x1 = y1; y1 = t; t = x2; x2 = y2; y2 = t;
  } else if (w2 < w0 && w2 < w1) {
    double t;
    t = w0; w0 = w2; w2 = t;
    t = x0; x0 = z0; z0 = t; t = x1; x1 = z1; z1 = t; t = x2; x2 = z2; z2 = t;
  }
  lambda1 = w2 < w1 ? w2 : w1;
  nrm[0] = x0;
  nrm[1] = x1;
  nrm[2] = x2;
}

__device__ __forceinline__ void fa_normal_from_cov(long long n, const double c[6], int axis, float nf[3]) {
  double nv[3] = {0.0, 0.0, 1.0};
  if (n >= 3) {
    double ev[3], l1;
    fa_eigvec(c, ev, l1);
    if (l1 > 1e-8) {
      nv[0] = ev[0];
      nv[1] = ev[1];
      nv[2] = ev[2];
    }
  }
  const double dot = axis == 0 ? nv[0] : (axis == 1 ? nv[1] : nv[2]);
  const double sgn = dot < 0.0 ? -1.0 : 1.0;
  nf[0] = (float)(sgn * nv[0]);
  nf[1] = (float)(sgn * nv[1]);
  nf[2] = (float)(sgn * nv[2]);
}

// normals_cell (te_kernels.hip) with the gather above.  fixup: only the cells k_fa_normals left to it (kExactNaN in the
// slope layer; given normals: in the roughness layer)
__global__ __launch_bounds__(TX* BY) void k_fa_exact(Geo g, any::NormalsJob a, const float* __restrict__ elev, const float* __restrict__ step,
                                                     float* __restrict__ slope, float* __restrict__ rough, float* __restrict__ trav,
                                                     float* __restrict__ onx, float* __restrict__ ony, float* __restrict__ onz, Region rg,
                                                     int fixup) {
  const int map = rg.map >= 0 ? rg.map : blockIdx.z;
  const size_t mo = (size_t)map * g.rows * g.cols;
  const int i = rg.i0 + blockIdx.x * TX + threadIdx.x, j = rg.j0 + blockIdx.y * BY + threadIdx.y;
  if (i >= rg.i1 || j >= rg.j1) return;
  const float* lay = elev + mo;
  const size_t o = mo + (size_t)j * g.rows + i;
  if (fixup && __builtin_bit_cast(unsigned, a.given_normals ? rough[o] : slope[o]) != kExactNaNBits) return;
  const float z0f = sanitize(lay[(size_t)j * g.rows + i]);
  const float qnan = __builtin_nanf("");
  float o_slope = qnan, o_rough = qnan, nf[3] = {qnan, qnan, qnan};
  MomL m;
  Mom mc;  // (the tails read its point count only)
  mom_zero(mc);
  double cov[6];
  if (a.given_normals) {  // RoughnessFilter::update as a stand-alone plugin: the normals come from the map
    nf[0] = onx[o];
    nf[1] = ony[o];
    nf[2] = onz[o];
    if (__builtin_isfinite(nf[0])) {  // RoughnessFilter.cpp:84
      fa_gather(m, g, a.dr, lay, i, j, (z0f == z0f) ? (double)z0f : 0.0);
      if (m.n >= 1) {
        mc.n = (int)m.n;
        fa_covariance(m, g.res, cov);
        o_rough = roughness_score(mc, cov, nf, a.rough_crit);
      } else {
        o_rough = a.rough_crit > 0.0 ? 1.0f : 0.0f;  // 0 points: 0 / SIZE_MAX = 0 (RoughnessFilter.cpp:117)
      }
    }
    rough[o] = o_rough;
    return;
  }
  if (z0f == z0f) {  // SlopeFilter.cpp:71, RoughnessFilter.cpp:84
    const double z0 = (double)z0f;
    fa_gather(m, g, a.dn, lay, i, j, z0);
    mc.n = (int)m.n;
    fa_covariance(m, g.res, cov);
    fa_normal_from_cov(m.n, cov, a.axis, nf);
    if (a.rank_rule && m.n >= 3 && rank_deficient(cov)) {  // UnitZ, towards the positive axis
      nf[0] = nf[1] = 0.0f;
      nf[2] = 1.0f;
    }
    o_slope = slope_score(nf[2], a.slope_crit);
    if (!a.same_disc) {
      fa_gather(m, g, a.dr, lay, i, j, z0);
      mc.n = (int)m.n;
      fa_covariance(m, g.res, cov);
    }
    o_rough = roughness_score(mc, cov, nf, a.rough_crit);
  }
  slope[o] = o_slope;
  rough[o] = o_rough;
  if (a.combine) {
    const float ta = a.w_slope * o_slope, tb = a.w_step * step[o], tc = a.w_rough * o_rough;
    const float tab = ta + tb;
    const float tabc = tab + tc;
    trav[o] = a.w_scale * tabc;
  }
  if (onx) {
    onx[o] = nf[0];
    ony[o] = nf[1];
    onz[o] = nf[2];
  }
}

// ------------------------------------------------------------------------------------------------
// Normals + slope + roughness in O(R) per cell: prefix moments of column segments
// ------------------------------------------------------------------------------------------------
// A block owns 64 centres (i) x 8 centre rows (j), two per thread, and walks the source columns j' within R of them.  Each
// column segment [i0 - H, i0 + 63 + H] (H: the widest run of either disc) is staged once as prefix sums of the per-cell
// moments -- count, sum t, sum t^2 as integers (t: row index local to the segment), sum z~, t z~, z~^2 in double with
// z~ = z - z_b (z_b: one valid centre elevation of the block) -- and every centre row reads its run of |j - j'| as two LDS
// reads per moment, shifted to the centre-local moments of te_cell.h (offsets di, dj; z - z0).  Precision:
// the indices are local to the segment and the elevations to the block, so no subtracted quantity grows with the row
// index or with the map's absolute elevation; what the moments lose is a few ulp of sums over at most 64 + 2H cells of
// (local index) x (local elevation).  Cells the tail cannot decide safely from that are left to k_fa_exact (kExactNaN in
// the slope layer, given normals: the roughness layer): a score within clip_band_* of its clip, fewer than 3 points or a
// middle eigenvalue below 1e-6 (the 1e-8 rule), two smallest eigenvalues closer than 1e-6 of the trace (the normal is
// ill-conditioned), a roughness residual below 1e-7 of the trace.
constexpr int TYN = 8;
constexpr int CPN = TYN / BY;

__device__ __forceinline__ void mom_clear(MomL& m) {
  m.n = m.si = m.sj = m.sii = m.sij = m.sjj = 0;
  m.sz = m.siz = m.sjz = m.szz = 0.0;
}

struct SegPrefix {
  const double *X, *Y, *W;
  const int *C, *A, *B;
};

// the run of disc D in column offset dj (|dj| = b) around segment-local centre ic, added to m in centre-local form
__device__ __forceinline__ void run_add(MomL& m, const Disc& D, int b, int dj, int i, int sa, int sb, int ic, double z0t, const SegPrefix& P) {
  if (b > D.R) return;
  const int h = disc_hw(D, b);
  if (h < 0) return;
  const int lo = (i - h < sa ? sa : i - h) - sa, hi = (i + h >= sb ? sb - 1 : i + h) - sa;
  const long long rn = P.C[hi + 1] - P.C[lo];
  if (rn == 0) return;
  const long long A = P.A[hi + 1] - P.A[lo], B = P.B[hi + 1] - P.B[lo];
  const double X = P.X[hi + 1] - P.X[lo], Y = P.Y[hi + 1] - P.Y[lo], W = P.W[hi + 1] - P.W[lo];
  const long long rsi = A - rn * ic;
  const long long rsii = B - 2 * (long long)ic * A + rn * ic * ic;
  const double rsz = X - (double)rn * z0t;
  const double rsiz = (Y - (double)ic * X) - z0t * (double)rsi;
  const double rszz = (W - z0t * X) - z0t * rsz;
  m.n += rn;
  m.si += rsi;
  m.sj += dj * rn;
  m.sii += rsii;
  m.sij += dj * rsi;
  m.sjj += (long long)dj * dj * rn;
  m.sz += rsz;
  m.siz += rsiz;
  m.sjz = fma((double)dj, rsz, m.sjz);
  m.szz += rszz;
}

__device__ __forceinline__ void ties_add(MomL& m, const Geo& g, const Disc& D, const float* __restrict__ lay, int i, int j, double zb, double z0t) {
  for (int t = 0; t < D.n_ties; ++t) {
    int di, dj;
    disc_tie(D, t, di, dj);
    const int ii = i + di, jj = j + dj;
    if (ii < 0 || ii >= g.rows || jj < 0 || jj >= g.cols || !tie_inside(g, D.r2, i, j, di, dj)) continue;
    const float z = lay[(size_t)jj * g.rows + ii];
    if (!__builtin_isfinite(z)) continue;
    const double dz = ((double)z - zb) - z0t;
    m.n += 1;
    m.si += di;
    m.sj += dj;
    m.sii += (long long)di * di;
    m.sij += (long long)di * dj;
    m.sjj += (long long)dj * dj;
    m.sz += dz;
    m.siz = fma((double)di, dz, m.siz);
    m.sjz = fma((double)dj, dz, m.sjz);
    m.szz = fma(dz, dz, m.szz);
  }
}

// roughness of the moments' covariance along normal nf (roughness_score before its clip); -1: fewer than 2 points.
// *unsafe: the residual is too small against the disc's extent for the prefix moments to decide it
__device__ __forceinline__ double fa_rough(const MomL& m, const double c[6], const float nf[3], bool* unsafe) {
  if (m.n < 2) return -1.0;
  const double a = (double)nf[0], b = (double)nf[1], cc = (double)nf[2];
  const double q0 = fma(c[0], a, fma(c[1], b, c[2] * cc));
  const double q1 = fma(c[1], a, fma(c[3], b, c[4] * cc));
  const double q2 = fma(c[2], a, fma(c[4], b, c[5] * cc));
  double q = fma(a, q0, fma(b, q1, cc * q2));
  *unsafe = !(q > 1e-7 * (c[0] + c[3] + c[5]));
  q = q < 0.0 ? 0.0 : q;  // (a NaN stays, and is `unsafe` above: the exact pass scores it 0 as the reference does)
  return sqrt(q * (double)m.n / (double)(m.n - 1));
}

__global__ __launch_bounds__(TX* BY) void k_fa_normals(Geo g, any::NormalsJob a, int seg, float band_slope, float band_rough,
                                                       const float* __restrict__ elev, const float* __restrict__ step, float* __restrict__ slope,
                                                       float* __restrict__ rough, float* __restrict__ trav, float* __restrict__ onx,
                                                       float* __restrict__ ony, float* __restrict__ onz, Region rg) {
  extern __shared__ double plds[];
  __shared__ double wsd[3][BY];
  __shared__ int wsi[3][BY];
  __shared__ int zb_idx;
  __shared__ float zb_val;
  const int map = rg.map >= 0 ? rg.map : blockIdx.z;
  const size_t mo = (size_t)map * g.rows * g.cols;
  const float* lay = elev + mo;
  const int i0 = rg.i0 + blockIdx.x * TX, j0 = rg.j0 + blockIdx.y * TYN;
  const int tid = threadIdx.y * TX + threadIdx.x, lane = threadIdx.x;
  const int i = i0 + threadIdx.x;
  const int hn = a.dn.R >= 0 ? disc_hw(a.dn, 0) : 0, hr = a.dr.R >= 0 ? disc_hw(a.dr, 0) : 0;
  const int H = hn > hr ? hn : hr;
  const int Rw = a.dn.R > a.dr.R ? a.dn.R : a.dr.R;
  const int sa = i0 - H < 0 ? 0 : i0 - H, sb = i0 + TX + H > g.rows ? g.rows : i0 + TX + H;
  const int n = sb - sa;
  double* PX = plds;
  double* PY = PX + (seg + 1);
  double* PW = PY + (seg + 1);
  int* PC = (int*)(PW + (seg + 1));
  int* PA = PC + (seg + 1);
  int* PB = PA + (seg + 1);
  const SegPrefix P = {PX, PY, PW, PC, PA, PB};
  const float qnan = __builtin_nanf("");
  float z0[CPN];
  bool live[CPN], want[CPN];
  if (tid == 0) zb_idx = 0x7fffffff;
  __syncthreads();
#pragma unroll
  for (int c = 0; c < CPN; ++c) {
    const int j = j0 + threadIdx.y + c * BY;
    live[c] = i < rg.i1 && j < rg.j1;
    z0[c] = live[c] ? sanitize(lay[(size_t)j * g.rows + i]) : qnan;
    want[c] = live[c] && (a.given_normals ? __builtin_isfinite(onx[mo + (size_t)j * g.rows + i]) : z0[c] == z0[c]);
    if (z0[c] == z0[c]) atomicMin(&zb_idx, c * TX * BY + tid);
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < CPN; ++c)
    if (z0[c] == z0[c] && c * TX * BY + tid == zb_idx) zb_val = z0[c];
  __syncthreads();
  const bool have_base = zb_idx != 0x7fffffff;  // (uniform)
  const double zb = have_base ? (double)zb_val : 0.0;
  if (!have_base) {  // no valid centre: nothing to gather for the chain; given normals: the exact pass
#pragma unroll
    for (int c = 0; c < CPN; ++c) {
      if (!live[c]) continue;
      const size_t o = mo + (size_t)(j0 + threadIdx.y + c * BY) * g.rows + i;
      if (a.given_normals) {
        rough[o] = want[c] ? __builtin_bit_cast(float, kExactNaNBits) : qnan;
      } else {
        slope[o] = qnan;
        rough[o] = qnan;
        if (a.combine) trav[o] = a.w_scale * ((a.w_slope * qnan + a.w_step * step[o]) + a.w_rough * qnan);
        if (onx) {
          onx[o] = qnan;
          ony[o] = qnan;
          onz[o] = qnan;
        }
      }
    }
    return;
  }
  double z0t[CPN];
  MomL mn[CPN], mr[CPN];
#pragma unroll
  for (int c = 0; c < CPN; ++c) {
    z0t[c] = z0[c] == z0[c] ? (double)z0[c] - zb : 0.0;  // (given normals, invalid centre: any origin, the covariance is the same)
    mom_clear(mn[c]);
    mom_clear(mr[c]);
  }
  const int chunk = (n + TX * BY - 1) / (TX * BY);
  const int t0 = tid * chunk < n ? tid * chunk : n, t1 = t0 + chunk < n ? t0 + chunk : n;
  const int jlo = j0 - Rw < 0 ? 0 : j0 - Rw;
  const int jhi = j0 + TYN - 1 + Rw >= g.cols ? g.cols - 1 : j0 + TYN - 1 + Rw;
#pragma unroll 1
  for (int jp = jlo; jp <= jhi; ++jp) {
    const float* col = lay + (size_t)jp * g.rows + sa;
    // the thread's chunk of the segment, then an exclusive scan of the chunk totals over the block
    int cc = 0, ca = 0, cb = 0;
    double cx = 0.0, cy = 0.0, cw = 0.0;
    for (int t = t0; t < t1; ++t) {
      const float z = col[t];
      if (!__builtin_isfinite(z)) continue;
      const double zt = (double)z - zb;
      cc += 1;
      ca += t;
      cb += t * t;
      cx += zt;
      cy = fma((double)t, zt, cy);
      cw = fma(zt, zt, cw);
    }
    int sc = cc, sa_ = ca, sb_ = cb;
    double sx = cx, sy = cy, sw = cw;
#pragma unroll
    for (int off = 1; off < TX; off <<= 1) {
      const int c1 = __shfl_up(sc, off), c2 = __shfl_up(sa_, off), c3 = __shfl_up(sb_, off);
      const double d1 = __shfl_up(sx, off), d2 = __shfl_up(sy, off), d3 = __shfl_up(sw, off);
      if (lane >= off) {
        sc += c1;
        sa_ += c2;
        sb_ += c3;
        sx += d1;
        sy += d2;
        sw += d3;
      }
    }
    __syncthreads();  // (the previous column's reads are done)
    if (lane == TX - 1) {
      wsi[0][threadIdx.y] = sc;
      wsi[1][threadIdx.y] = sa_;
      wsi[2][threadIdx.y] = sb_;
      wsd[0][threadIdx.y] = sx;
      wsd[1][threadIdx.y] = sy;
      wsd[2][threadIdx.y] = sw;
    }
    __syncthreads();
    // exclusive prefix of this thread's chunk
    sc -= cc;
    sa_ -= ca;
    sb_ -= cb;
    sx -= cx;
    sy -= cy;
    sw -= cw;
    for (int w = 0; w < (int)threadIdx.y; ++w) {
      sc += wsi[0][w];
      sa_ += wsi[1][w];
      sb_ += wsi[2][w];
      sx += wsd[0][w];
      sy += wsd[1][w];
      sw += wsd[2][w];
    }
    if (tid == 0) {
      PC[0] = PA[0] = PB[0] = 0;
      PX[0] = PY[0] = PW[0] = 0.0;
    }
    for (int t = t0; t < t1; ++t) {
      const float z = col[t];
      if (__builtin_isfinite(z)) {
        const double zt = (double)z - zb;
        sc += 1;
        sa_ += t;
        sb_ += t * t;
        sx += zt;
        sy = fma((double)t, zt, sy);
        sw = fma(zt, zt, sw);
      }
      PC[t + 1] = sc;
      PA[t + 1] = sa_;
      PB[t + 1] = sb_;
      PX[t + 1] = sx;
      PY[t + 1] = sy;
      PW[t + 1] = sw;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < CPN; ++c) {
      if (!want[c]) continue;
      const int j = j0 + threadIdx.y + c * BY;
      const int dj = jp - j, b = dj < 0 ? -dj : dj;
      run_add(mn[c], a.dn, b, dj, i, sa, sb, i - sa, z0t[c], P);
      if (!a.same_disc) run_add(mr[c], a.dr, b, dj, i, sa, sb, i - sa, z0t[c], P);
    }
  }
#pragma unroll
  for (int c = 0; c < CPN; ++c) {
    if (!live[c]) continue;
    const int j = j0 + threadIdx.y + c * BY;
    const size_t o = mo + (size_t)j * g.rows + i;
    float o_slope = qnan, o_rough = qnan, nf[3] = {qnan, qnan, qnan};
    bool exact = false;
    double cov[6];
    if (a.given_normals) {
      if (want[c]) {
        ties_add(mn[c], g, a.dr, lay, i, j, zb, z0t[c]);
        nf[0] = onx[o];
        nf[1] = ony[o];
        nf[2] = onz[o];
        if (mn[c].n == 0) {
          o_rough = a.rough_crit > 0.0 ? 1.0f : 0.0f;  // 0 points: 0 / SIZE_MAX = 0 (RoughnessFilter.cpp:117)
        } else {
          fa_covariance(mn[c], g.res, cov);
          bool unsafe = false;
          const double r = fa_rough(mn[c], cov, nf, &unsafe);
          if (r < 0.0) {
            o_rough = 0.0f;  // one point: 0/0 (roughness_score)
          } else {
            const double raw = 1.0 - r / a.rough_crit;
            exact = unsafe || (a.rough_crit > 0.0 && fabs(raw) <= band_rough);
            o_rough = r < a.rough_crit ? (float)raw : 0.0f;
          }
        }
      }
      rough[o] = exact ? __builtin_bit_cast(float, kExactNaNBits) : o_rough;
      continue;
    }
    if (want[c]) {
      ties_add(mn[c], g, a.dn, lay, i, j, zb, z0t[c]);
      fa_covariance(mn[c], g.res, cov);
      double ev[3] = {0.0, 0.0, 1.0}, l1 = 0.0;
      exact = mn[c].n < 3;
      if (!exact) {
        fa_eigvec(cov, ev, l1);
        const double tr = cov[0] + cov[3] + cov[5];
        const double q0 = fma(cov[0], ev[0], fma(cov[1], ev[1], cov[2] * ev[2]));
        const double q1 = fma(cov[1], ev[0], fma(cov[3], ev[1], cov[4] * ev[2]));
        const double q2 = fma(cov[2], ev[0], fma(cov[4], ev[1], cov[5] * ev[2]));
        const double l0 = fma(ev[0], q0, fma(ev[1], q1, ev[2] * q2));  // (Rayleigh quotient: the smallest eigenvalue)
        exact = !(l1 > 1e-6) || !(l1 - l0 > 1e-6 * tr);
      }
      if (!exact) {
        const double dot = a.axis == 0 ? ev[0] : (a.axis == 1 ? ev[1] : ev[2]);
        const double sgn = dot < 0.0 ? -1.0 : 1.0;
        nf[0] = (float)(sgn * ev[0]);
        nf[1] = (float)(sgn * ev[1]);
        nf[2] = (float)(sgn * ev[2]);
        const double sl = acos((double)nf[2]);  // SlopeFilter.cpp:74
        const double raw = 1.0 - sl / a.slope_crit;
        exact = a.slope_crit > 0.0 && fabs(raw) <= band_slope;
        o_slope = sl < a.slope_crit ? (float)raw : 0.0f;
        const MomL& mq = a.same_disc ? mn[c] : mr[c];
        if (!a.same_disc) {
          ties_add(mr[c], g, a.dr, lay, i, j, zb, z0t[c]);
          fa_covariance(mr[c], g.res, cov);
        }
        bool unsafe = false;
        const double r = fa_rough(mq, cov, nf, &unsafe);
        if (r < 0.0) {
          o_rough = 0.0f;
        } else {
          const double rr = 1.0 - r / a.rough_crit;
          exact = exact || unsafe || (a.rough_crit > 0.0 && fabs(rr) <= band_rough);
          o_rough = r < a.rough_crit ? (float)rr : 0.0f;
        }
      }
    }
    if (exact) {
      slope[o] = __builtin_bit_cast(float, kExactNaNBits);
      continue;
    }
    slope[o] = o_slope;
    rough[o] = o_rough;
    if (a.combine) {
      const float ta = a.w_slope * o_slope, tb = a.w_step * step[o], tc = a.w_rough * o_rough;
      const float tab = ta + tb;
      const float tabc = tab + tc;
      trav[o] = a.w_scale * tabc;
    }
    if (onx) {
      onx[o] = nf[0];
      ony[o] = nf[1];
      onz[o] = nf[2];
    }
  }
}

// LDS of k_fa_normals' prefix sums (kMaxLds + 1: does not fit); *seg: the longest segment
size_t normals_lds(const Geo& g, const any::NormalsJob& a, int* seg) {
  auto hw0 = [](const Disc& d) -> long long { return d.R >= 0 ? (d.any ? d.any_hw0 : d.hw[0]) : 0; };
  const long long H = hw0(a.dn) > hw0(a.dr) ? hw0(a.dn) : hw0(a.dr);
  const long long s = (long long)TX + 2 * H < (long long)g.rows ? (long long)TX + 2 * H : (long long)g.rows;
  *seg = (int)(s < (1 << 20) ? s : 1 << 20);
  const long long bytes = (s + 1) * (3 * (long long)sizeof(double) + 3 * (long long)sizeof(int));
  return bytes > (long long)kMaxLds ? kMaxLds + 1 : (size_t)bytes;
}

// LDS of a step kernel's tables for disc d on this map, in bytes (kMaxLds + 1: does not fit); *stride: floats per level
size_t step_lds(const Geo& g, const Disc& d, bool score, int* stride) {
  const long long H = d.R >= 0 ? (d.any ? d.any_hw0 : d.hw[0]) : 0;
  const long long seg = (long long)TX + 2 * H < (long long)g.rows ? (long long)TX + 2 * H : (long long)g.rows;
  const long long wmax = 2 * H + 1 < seg ? 2 * H + 1 : seg;
  int levels = 1;
  while ((1ll << levels) <= wmax) ++levels;
  *stride = (int)(seg < (1 << 20) ? seg : 1 << 20);
  const long long bytes = score ? (long long)levels * seg * 4 + (seg + 1) * 4 : 2ll * levels * seg * 4;
  return bytes > (long long)kMaxLds ? kMaxLds + 1 : (size_t)bytes;
}

}  // namespace

namespace any {

hipError_t step_height(const Geo& g, const Disc& d, const float* elev, float* sh, const Region& r, hipStream_t s) {
  if (r.i1 <= r.i0 || r.j1 <= r.j0) return hipSuccess;
  int stride = 0;
  const size_t lds = step_lds(g, d, false, &stride);
  const unsigned nz = (unsigned)(r.map >= 0 ? 1 : g.batch);
  if (lds <= kMaxLds) {
    const dim3 grid((unsigned)((r.i1 - r.i0 + TX - 1) / TX), (unsigned)((r.j1 - r.j0 + TYB - 1) / TYB), nz);
    hipLaunchKernelGGL(k_fa_step_height, grid, dim3(TX, BY), lds, s, g, d, stride, elev, sh, r);
  } else {
    const dim3 grid((unsigned)((r.i1 - r.i0 + TX - 1) / TX), (unsigned)((r.j1 - r.j0 + BY - 1) / BY), nz);
    hipLaunchKernelGGL(k_fa_step_exact<false>, grid, dim3(TX, BY), 0, s, g, d, 0.0, 1, elev, sh, r);
  }
  return hipGetLastError();
}

hipError_t step_score(const Geo& g, const Disc& d, double crit, int ncrit, const float* sh, float* out, const Region& r, hipStream_t s) {
  if (r.i1 <= r.i0 || r.j1 <= r.j0) return hipSuccess;
  int stride = 0;
  const size_t lds = step_lds(g, d, true, &stride);
  const unsigned nz = (unsigned)(r.map >= 0 ? 1 : g.batch);
  if (lds <= kMaxLds) {
    const dim3 grid((unsigned)((r.i1 - r.i0 + TX - 1) / TX), (unsigned)((r.j1 - r.j0 + TYB - 1) / TYB), nz);
    hipLaunchKernelGGL(k_fa_step_score, grid, dim3(TX, BY), lds, s, g, d, stride, crit, ncrit, sh, out, r);
  } else {
    const dim3 grid((unsigned)((r.i1 - r.i0 + TX - 1) / TX), (unsigned)((r.j1 - r.j0 + BY - 1) / BY), nz);
    hipLaunchKernelGGL(k_fa_step_exact<true>, grid, dim3(TX, BY), 0, s, g, d, crit, ncrit, sh, out, r);
  }
  return hipGetLastError();
}

hipError_t normals(const Geo& g, const NormalsJob& a, const Layers& L, float* nx, float* ny, float* nz, const Region& r, hipStream_t s) {
  if (r.i1 <= r.i0 || r.j1 <= r.j0) return hipSuccess;
  const unsigned nz_ = (unsigned)(r.map >= 0 ? 1 : g.batch);
  const dim3 grid((unsigned)((r.i1 - r.i0 + TX - 1) / TX), (unsigned)((r.j1 - r.j0 + BY - 1) / BY), nz_);
  int seg = 0;
  // (TE_OPT_NORMALS_RANK_RULE lives in the exact gather only; so does a segment whose prefix sums outgrow 64 KiB)
  const size_t lds = normals_lds(g, a, &seg);
  if (!a.rank_rule && lds <= kMaxLds) {
    const dim3 gridn((unsigned)((r.i1 - r.i0 + TX - 1) / TX), (unsigned)((r.j1 - r.j0 + TYN - 1) / TYN), nz_);
    hipLaunchKernelGGL(k_fa_normals, gridn, dim3(TX, BY), lds, s, g, a, seg, clip_band_slope(a.slope_crit), clip_band_rough(a.rough_crit),
                       L.elev, L.step, L.slope, L.rough, L.trav, nx, ny, nz, r);
    hipLaunchKernelGGL(k_fa_exact, grid, dim3(TX, BY), 0, s, g, a, L.elev, L.step, L.slope, L.rough, L.trav, nx, ny, nz, r, 1);
  } else {
    hipLaunchKernelGGL(k_fa_exact, grid, dim3(TX, BY), 0, s, g, a, L.elev, L.step, L.slope, L.rough, L.trav, nx, ny, nz, r, 0);
  }
  return hipGetLastError();
}

}  // namespace any
}  // namespace te
