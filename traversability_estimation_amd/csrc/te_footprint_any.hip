// te_footprint_any.hip -- the circular footprint pass at any reach (TraversabilityMap::isTraversable(center, radiusMax,
// traversability, radiusMin), TraversabilityMap.cpp:654-746, for every cell).
//
// The shape-specialised sum kernels (te_footprint*.hip) hold the disc in an LDS ring or in compile-time run tables and
// serve reaches up to 20 cells.  This route serves every reach, from the tables of te_fp_table.h (runs, ties, spiral order;
// clipped to the map), and is what launch_footprint picks above 20 cells, with TE_OPT_FP_ANY_REACH = 1, or at any reach for
// a traversability layer without the bound the double kernels need (te_fp_route.h fp_packed_ok: a layer written from
// outside, a large or negative weight, a large default).  The mask kernel (k_fp_mask) runs before it, unchanged.
//
//   k_fpa_prefix  column prefix sums along the contiguous i axis, per map and column: P[i] = sum of T' over rows < i in
//                 double (T' = traversability, traversability_default where it is not finite, :719-724) and C[i] = the
//                 number of untraversable cells among them, as an integer.  One wavefront per column, a 64-wide scan per
//                 step.
//   k_fpa_sum     one lane per cell: the disc's row runs cost two loads each from P and C (O(R) per cell, not O(R^2)),
//                 the tie offsets are decided per centre with isInside's formula and read directly.  No untraversable
//                 cell: the mean of T' (:732-735).  Otherwise the value of the first untraversable cell in SpiralIterator
//                 order (:687-717): 0 when radiusMin is 0 or the cell lies within it; an untraversable cell in the rings
//                 that lie within radiusMin is found from C in O(R) (inner disc); else the wavefront walks the spiral
//                 table from the end of the inner disc, 64 entries per step, one disc at a time.
// The untraversable count is exact (integers) whatever the disc's size or the values of the traversability layer.  The sum
// is in double, but as differences of a prefix that runs down the WHOLE column: its error is about 2^-52 times the column's
// sum of |T'| per run, not local to the disc (include/travgpu.h, te_run_footprint, states the range this supports).
#include "te_internal.h"

#include "te_fp_table.h"
#include "te_geom.h"

namespace te {
namespace {

constexpr int kLanes = 64;
constexpr int kRowsPerBlock = 4;  // wavefronts (= map columns j) per block

__device__ __forceinline__ float qnanf() { return __builtin_nanf(""); }

// Prefix sums of the columns [j0, j1) of maps map0 + blockIdx.z: psum / pcnt [map][col][rows + 1], entry 0 is 0.
__global__ __launch_bounds__(kLanes* kRowsPerBlock) void k_fpa_prefix(Geo g, const float* __restrict__ trav,
                                                                    const uint8_t* __restrict__ untrav, double* __restrict__ psum,
                                                                    unsigned* __restrict__ pcnt, double def, int map0, int j0,
                                                                    int j1) {
  const int lane = threadIdx.x & (kLanes - 1);
  const int j = j0 + (int)blockIdx.x * kRowsPerBlock + (int)(threadIdx.x / kLanes);
  if (j >= j1) return;  // (a whole wavefront: no barrier below)
  const size_t col = (size_t)(map0 + (int)blockIdx.z) * g.cols + j;
  const size_t src = col * g.rows;
  const size_t dst = col * (size_t)(g.rows + 1);
  if (lane == 0) {
    psum[dst] = 0.0;
    pcnt[dst] = 0u;
  }
  double carry = 0.0;
  unsigned ccarry = 0u;
  for (int i0 = 0; i0 < g.rows; i0 += kLanes) {
    const int i = i0 + lane;
    double v = 0.0;
    unsigned u = 0u;
    if (i < g.rows) {
      const float t = trav[src + i];
      v = __builtin_isfinite(t) ? (double)t : def;
      u = untrav[src + i] ? 1u : 0u;
    }
#pragma unroll
    for (int d = 1; d < kLanes; d <<= 1) {
      const double ov = __shfl_up(v, d);
      const unsigned ou = __shfl_up(u, d);
      if (lane >= d) {
        v += ov;
        u += ou;
      }
    }
    v += carry;
    u += ccarry;
    if (i < g.rows) {
      psum[dst + i + 1] = v;
      pcnt[dst + i + 1] = u;
    }
    carry = __shfl(v, kLanes - 1);
    ccarry = __shfl(u, kLanes - 1);
  }
}

struct AnyArgs {
  const double* psum;
  const unsigned* pcnt;
  const int* ints;       // [0, R]: run half-widths hw[|dj|]; [R + 1, R + 1 + inner_R]: those of the inner disc; then the ties (di, dj)
  const int4* spiral;    // FpEntry {di, dj, ring, tie}, SpiralIterator order
  int n_spiral;
  int R, inner_R, n_ties;
  int k_inner;           // spiral entries of the inner disc (rings 0 .. d, all of them: a prefix of the table)
  double r2, rmin, rmax, def;
  int map0, i0, j0, i1, j1;  // output rectangle (every map of the launch)
};

__global__ __launch_bounds__(kLanes* kRowsPerBlock) void k_fpa_sum(Geo g, AnyArgs a, const float* __restrict__ trav,
                                                                 const uint8_t* __restrict__ untrav, float* __restrict__ footprint) {
  const int lane = threadIdx.x;
  const int j = a.j0 + (int)blockIdx.y * kRowsPerBlock + (int)threadIdx.y;
  if (j >= a.j1) return;  // (a whole wavefront: no barrier below)
  const int i = a.i0 + (int)blockIdx.x * kLanes + lane;
  const bool valid = i < a.i1;
  const int map = a.map0 + (int)blockIdx.z;
  const size_t mo = (size_t)map * g.rows * g.cols;
  const size_t pstride = (size_t)(g.rows + 1);
  const size_t pmo = (size_t)map * g.cols * pstride;
  const int* __restrict__ hw = a.ints;
  const int* __restrict__ ihw = a.ints + a.R + 1;
  const int* __restrict__ ties = a.ints + a.R + 1 + (a.inner_R + 1);

  // sum of T', untraversable cells and cells of the disc within the rows [i - h, i + h] of columns j +- dj
  double S = 0.0;
  unsigned U = 0u;
  int n = 0;
  auto add_runs = [&](const int* __restrict__ h_of, int R, double& s, unsigned& u, int& cnt) __attribute__((always_inline)) {
    const int dlo = j - R < 0 ? -j : -R, dhi = j + R >= g.cols ? g.cols - 1 - j : R;
    for (int dj = dlo; dj <= dhi; ++dj) {
      const int h = h_of[dj < 0 ? -dj : dj];  // uniform
      if (h < 0) continue;
      const int lo = i - h > 0 ? i - h : 0;
      const int hi = i + h < g.rows - 1 ? i + h : g.rows - 1;
      if (hi < lo) continue;
      const size_t pc = pmo + (size_t)(j + dj) * pstride;
      s += a.psum[pc + hi + 1] - a.psum[pc + lo];
      u += a.pcnt[pc + hi + 1] - a.pcnt[pc + lo];
      cnt += hi - lo + 1;
    }
  };
  if (a.R >= 0) add_runs(hw, a.R, S, U, n);
  // cells on the circle: SpiralIterator::isInside per centre
  for (int t = 0; t < a.n_ties; ++t) {
    const int ii = i + ties[2 * t], jj = j + ties[2 * t + 1];
    if (!valid || ii < 0 || ii >= g.rows || jj < 0 || jj >= g.cols) continue;
    const double dx = cell_x(g, ii) - cell_x(g, i), dy = cell_y(g, jj) - cell_y(g, j);
    if (dx * dx + dy * dy <= a.r2) {
      const size_t o = mo + (size_t)jj * g.rows + ii;
      const float tv = trav[o];
      S += __builtin_isfinite(tv) ? (double)tv : a.def;
      U += untrav[o] ? 1u : 0u;
      n += 1;
    }
  }
  float out = qnanf();
  if (U == 0u) {
    out = (float)(S / (double)n);  // :732-735
  } else if (a.rmin == 0.0) {
    out = 0.0f;  // :694-704: radiusMin 0 makes the value 0 whichever cell is the first
  }
  bool need = valid && U != 0u && a.rmin != 0.0;
  // the inner disc: an untraversable cell in the rings within radiusMin makes the value 0; otherwise its sum and cell
  // count start the walk
  double Sin = 0.0;
  int nin = 0;
  if (a.inner_R >= 0 && __any(need)) {
    unsigned Uin = 0u;
    add_runs(ihw, a.inner_R, Sin, Uin, nin);
    if (need && Uin != 0u) {
      out = 0.0f;
      need = false;
    }
  }
  // the discs whose first untraversable cell lies further out, one at a time with the whole wavefront
  unsigned long long rest = __ballot(need);
  while (rest != 0ull) {
    const int l = __builtin_ctzll(rest);
    rest &= rest - 1ull;
    const int ic = __shfl(i, l);
    const double acc0 = __shfl(Sin, l);
    const int cnt0 = __shfl(nin, l);
    double acc = 0.0;
    int cnt = 0;
    float oc = qnanf();
    for (int k0 = a.k_inner; k0 < a.n_spiral; k0 += kLanes) {
      const int k = k0 + lane;
      int4 e = make_int4(0, 0, 0, 0);
      if (k < a.n_spiral) e = a.spiral[k];
      const int ii = ic + e.x, jj = j + e.y;
      bool in = k < a.n_spiral && ii >= 0 && ii < g.rows && jj >= 0 && jj < g.cols;
      if (in && e.w) {
        const double dx = cell_x(g, ii) - cell_x(g, ic), dy = cell_y(g, jj) - cell_y(g, j);
        in = dx * dx + dy * dy <= a.r2;
      }
      double v = 0.0;
      bool u = false;
      if (in) {
        const size_t o = mo + (size_t)jj * g.rows + ii;
        const float tv = trav[o];
        v = __builtin_isfinite(tv) ? (double)tv : a.def;
        u = untrav[o] != 0;
      }
      const unsigned long long bm = __ballot(in && u);
      if (bm != 0ull) {
        const int first = __builtin_ctzll(bm);
        const int ring_first = __shfl(e.z, first);
        const double ru = (double)ring_first * g.res;  // getCurrentRadius()
        if (ru <= a.rmin) {                            // :694-704
          oc = 0.0f;
          break;
        }
        const bool before = in && lane < first;
        acc += before ? v : 0.0;
        cnt += __popcll(__ballot(before));
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
        double tsum = acc0 + acc;
        const int ncells = cnt0 + cnt;
        const double factor = ((ru - a.rmin) / (a.rmax - a.rmin) + 1.0) / 2.0;  // :705-711
        tsum *= factor / ncells;
        oc = (float)tsum;
        break;
      }
      acc += in ? v : 0.0;
      cnt += __popcll(__ballot(in));
    }
    if (lane == l) out = oc;  // (the disc holds an untraversable cell beyond the inner disc, so the walk set oc)
  }
  if (valid) footprint[mo + (size_t)j * g.rows + i] = out;
}

}  // namespace

// rf: the output cells of map rf->map (a region run: the changed cells grown by the mask's 3 cells and the reach), nullptr:
// every cell of every map.  The prefix sums always cover every column of the maps of the launch: a caller may have written
// the traversability layer anywhere since the last pass (te_device_ptr), and one streaming pass costs little beside the sum.
hipError_t launch_footprint_any(const Geo& g, const FootprintParams& p, const Layers& L, const Region* rf, hipStream_t s) {
  if (!p.any_spiral || !p.any_psum || !p.any_pcnt) return hipErrorInvalidValue;
  const int nmaps = rf ? 1 : g.batch;
  const int map0 = rf ? rf->map : 0;
  {
    const dim3 grid((unsigned)((g.cols + kRowsPerBlock - 1) / kRowsPerBlock), 1u, (unsigned)nmaps);
    hipLaunchKernelGGL(k_fpa_prefix, grid, dim3(kLanes * kRowsPerBlock), 0, s, g, L.trav, L.untrav, p.any_psum, p.any_pcnt, p.def,
                       map0, 0, g.cols);
  }
  AnyArgs a;
  a.psum = p.any_psum;
  a.pcnt = p.any_pcnt;
  a.ints = p.any_ints;
  a.spiral = reinterpret_cast<const int4*>(p.any_spiral);
  a.n_spiral = p.any_n_spiral;
  a.R = p.any_R;
  a.inner_R = p.any_inner_R;
  a.n_ties = p.any_n_ties;
  a.k_inner = p.any_k_inner;
  a.r2 = p.rmax * p.rmax;
  a.rmin = p.rmin;
  a.rmax = p.rmax;
  a.def = p.def;
  a.map0 = map0;
  a.i0 = rf ? rf->i0 : 0;
  a.j0 = rf ? rf->j0 : 0;
  a.i1 = rf ? rf->i1 : g.rows;
  a.j1 = rf ? rf->j1 : g.cols;
  if (a.i1 <= a.i0 || a.j1 <= a.j0) return hipGetLastError();
  const dim3 grid((unsigned)((a.i1 - a.i0 + kLanes - 1) / kLanes), (unsigned)((a.j1 - a.j0 + kRowsPerBlock - 1) / kRowsPerBlock),
                  (unsigned)nmaps);
  hipLaunchKernelGGL(k_fpa_sum, grid, dim3(kLanes, kRowsPerBlock), 0, s, g, a, L.trav, L.untrav, L.footprint);
  return hipGetLastError();
}

}  // namespace te
