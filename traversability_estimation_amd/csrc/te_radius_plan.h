// te_radius_plan.h -- te_run_radius_filter (MeanInRadiusFilter / MinInRadiusFilter) as a plan: plain C++, no HIP, shared
// with the CPU test (tests/cpu/radius_plan_check.cpp).  Which kernel a call takes, the LDS of the sliding kernels, and the
// predicate under which the sliding Mean may add in another order than the contract's.
//
// The kernels (te_radius.hip).  A workgroup of 256 lanes owns kTX x kTY = 64 x 16 centres (rows are contiguous in memory).
//   gather        every centre walks its window in the contract's order (row offset ascending, column offset ascending)
//                 with bounds-checked loads from global memory.  Exact on every input, O(r^2) per cell.
//   sliding Min   per source column the segment [i0 - H, i0 + 63 + H] is staged once as a sparse table of range minima and a
//                 centre reads the run of a column as two LDS reads: O(r) per cell.  A minimum does not depend on the order.
//   sliding Mean  the same segments as prefix sums in double and prefix counts of their finite cells; a run is a difference of
//                 two prefixes.  That is another summation order than the contract's, so a workgroup takes it only when
//                 order_free() holds for every cell it can read, and otherwise runs the gather for its centres.
//
// The predicate.  Every finite non-zero float of exponents in [emin, emax] (denormals count as -126) is an integer multiple of
// 2^(emin - 23) and smaller in magnitude than 2^(emax + 1).  A sum of at most n of them, any subset in any order, is a multiple
// of the same unit and smaller than 2^(emax + 1 + ceil(log2 n)): it is a double exactly -- and so is every intermediate of
// every order -- when   emax + 1 + ceil(log2 n) - (emin - 23) <= 53.   Then the in-order sum, the prefixes, their differences
// and the sum over the columns are all the exact real sum, a zero sum is +0.0 on both routes (x + (-x) and x - x are +0.0 in
// round-to-nearest, and 0.0 + -0.0 is +0.0), and the two routes give the same bits.  n is the larger of the disc's cells (ties
// included) and the staged segment's length.
//
// Route by plan (TE_OPT_RADIUS_ROUTE = 0): the sliding kernel wherever it can run, kSlideMinCells = 0.  Measured on a 4096 x 4096
// map at 0, 0.5, 1.5, 3, 9 and 20 cells (tools/radius_filter_bench.py, profiles/radius_filter_bench.json): the
// sliding kernels beat the gather at every one of them, Mean 0.22 against 0.79 ms at 0 cells, 1.47 against 8.57 ms at 20 -- against
// the gather as it is built, which loads from global memory; a gather that stages a tile with its halo in LDS was not built and
// might move the crossover at the smallest radii.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TE_RADIUS_HD __host__ __device__ inline
#else
#define TE_RADIUS_HD inline
#endif

namespace te {
namespace radius {

constexpr int kTX = 64, kTY = 16, kWaves = 4, kThreads = kTX * kWaves;
constexpr size_t kMaxLds = 64 * 1024;
constexpr unsigned kMaxGridY = 65535;
// discs whose runs reach fewer cells than this go to the gather under TE_OPT_RADIUS_ROUTE = 0 (0: none; measured, see above)
constexpr int kSlideMinCells = 0;

enum Op { kMean = 1, kMin = 2 };
enum Route { kRouteSlide = 1, kRouteGather = 2 };

// binary exponent of a finite non-zero float given by its bits; denormals count as -126
TE_RADIUS_HD int float_exponent(uint32_t bits) {
  const int e = (int)((bits >> 23) & 0xffu);
  return e == 0 ? -126 : e - 127;
}
inline int ceil_log2(unsigned long long n) {
  int k = 0;
  while (k < 63 && (1ull << k) < n) ++k;
  return k;
}
// emax < emin: no finite non-zero cell was seen, every sum is zero
TE_RADIUS_HD bool order_free(int emax, int emin, int log2n) { return emax < emin || emax + 1 + log2n - (emin - 23) <= 53; }

// The window table of one call, as the kernels read it: hw[0 .. R] (the disc is symmetric: the run of row offset di is
// [-hw[|di|], hw[|di|]] in dj), then the ties as (di, dj) pairs sorted by di, then dj -- the contract's order.
struct Shape {
  int R;       // -1: no run
  int hw0;     // hw[0] (0 without runs)
  int reach;   // largest |offset| of runs and ties
  int n_ties;
  long long npoints;  // cells of the runs
};

// rows of the segment a workgroup stages around its 64 centres
inline long long segment_len(int rows, int hw0) {
  const long long s = (long long)kTX + 2 * (long long)hw0;
  return s < rows ? s : rows;
}
inline int min_levels(int rows, int hw0) {
  const long long seg = segment_len(rows, hw0), w = 2 * (long long)hw0 + 1 < seg ? 2 * (long long)hw0 + 1 : seg;
  int levels = 1;
  while ((1ll << levels) <= w) ++levels;
  return levels;
}
// dynamic LDS of the sliding kernels in bytes (kMaxLds + 1: does not fit)
inline size_t min_lds_bytes(int rows, int hw0) {
  const long long b = (long long)min_levels(rows, hw0) * segment_len(rows, hw0) * (long long)sizeof(float);
  return b > (long long)kMaxLds ? kMaxLds + 1 : (size_t)b;
}
// prefix sums and counts of the segment (seg + 1 each), the two scan buffers of 256 partial sums and counts, emax / emin
inline size_t mean_lds_bytes(int rows, int hw0) {
  const long long b = (segment_len(rows, hw0) + 1 + 2 * kThreads) * (long long)(sizeof(double) + sizeof(int)) + 2 * (long long)sizeof(int);
  return b > (long long)kMaxLds ? kMaxLds + 1 : (size_t)b;
}

struct Plan {
  int route;
  size_t lds_bytes;  // of the sliding kernel (0 on the gather)
  int seg;           // rows of a staged segment
  int levels;        // of the Min tables
  int log2n;         // ceil(log2 n) of the predicate
  unsigned grid_x, grid_y;
};

// option: TE_OPT_RADIUS_ROUTE -- 0 by plan, 1 the sliding kernel wherever it can run, 2 the gather always
inline Plan plan(int op, int rows, int cols, const Shape& s, int option) {
  Plan p;
  memset(&p, 0, sizeof(p));
  const size_t lds = op == kMin ? min_lds_bytes(rows, s.hw0) : mean_lds_bytes(rows, s.hw0);
  const unsigned gy = (unsigned)(((long long)cols + kTY - 1) / kTY);
  bool slide = option != 2 && lds <= kMaxLds && gy <= kMaxGridY;
  if (option == 0 && s.hw0 < kSlideMinCells) slide = false;
  p.route = slide ? kRouteSlide : kRouteGather;
  p.lds_bytes = slide ? lds : 0;
  p.seg = (int)segment_len(rows, s.hw0);
  p.levels = min_levels(rows, s.hw0);
  const unsigned long long pts = (unsigned long long)s.npoints + (unsigned long long)s.n_ties, seg = (unsigned long long)p.seg;
  p.log2n = ceil_log2(pts > seg ? pts : seg);
  p.grid_x = (unsigned)((rows + kTX - 1) / kTX);
  if (slide) {
    p.grid_y = gy;
  } else {  // one centre per lane, 4 columns per workgroup; a taller grid than kMaxGridY is walked in strides
    const unsigned g4 = (unsigned)(((long long)cols + kWaves - 1) / kWaves);
    p.grid_y = g4 > kMaxGridY ? kMaxGridY : g4;
  }
  return p;
}

// a radius beyond the map's rows + cols + 2 cells selects every cell of the map from every centre, as does that bound: its
// disc has no cell of the map on its circle (|di| < rows and |dj| < cols give di^2 + dj^2 < (rows + cols + 2)^2), and the
// table stays O(rows + cols) whatever the radius is
inline double bounded_radius(double radius, double res, int rows, int cols) {
  const double cap = ((double)rows + (double)cols + 2.0) * res;
  return radius < cap ? radius : cap;
}

}  // namespace radius
}  // namespace te
