// te_distance.h -- the per-cell routines of te_run_distance (include/travgpu.h: the exact Euclidean distance to the nearest
// seed): plain C++ that compiles for the host and the device.  The kernels (te_distance.hip) instantiate exactly this code, and
// the CPU test (tests/cpu/distance_plan_check.cpp) runs it against brute force.
//
// The transform is two separable passes, both exact in integers:
//   pass 1   g(i, j) = the distance in cells from (i, j) to the nearest seed of its column j (along i, the contiguous axis),
//            saturated at R + 1.  A wavefront holds the seeds of 64 consecutive rows as one 64-bit mask (a ballot); a cell is
//            one bit of it, and what lies outside the chunk arrives as two numbers: the distance from the chunk's first cell
//            to the nearest seed before it, and from its last cell to the nearest seed after it (column_nearest).
//   pass 2   d2(i, j) = min over dj in [-R, R] of g(i, j + dj)^2 + dj^2, walked outward from dj = 0 and ended as soon as dj^2
//            cannot improve the best found so far, which starts at cap2 + 1 (row_min).  (R + 1)^2 > cap2, so a saturated g
//            never wins.  g <= 32768 and dj <= 32767: every sum fits in 32 bits.
// Nothing is decided in floating point before the final sqrt (value_of).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TE_DIST_HD __host__ __device__ inline
#else
#define TE_DIST_HD inline
#endif

namespace te {
namespace distance {

// the modes of include/travgpu.h (TE_DISTANCE_*; te_distance_api.hip holds them equal)
enum Mode { kBelow = 1, kAbove = 2, kNanIsSeed = 4 };
constexpr int kLanes = 64;
// "no seed on that side": larger than every distance in cells, small enough to add a lane index to
constexpr int kNone = 1 << 29;

// ThresholdFilter's comparisons on the float: v == threshold is no seed in either mode
TE_DIST_HD bool is_seed(float v, int mode, float threshold) {
  if (v != v) return (mode & kNanIsSeed) != 0;
  return (mode & 3) == kBelow ? v < threshold : v > threshold;
}

// The cell is bit `l` of `m`, the seeds of the 64 rows of its chunk.  before: the distance from bit 0 to the nearest seed
// before the chunk (>= 1, kNone: none); after: from bit 63 to the nearest seed after it.  The result is min(distance, sat).
TE_DIST_HD int column_nearest(uint64_t m, int l, int before, int after, int sat) {
  int d = l + before;
  const int a = (kLanes - 1 - l) + after;
  d = a < d ? a : d;
  const uint64_t lo = m & (~0ull >> (kLanes - 1 - l));  // bits 0 .. l
  if (lo) {
    const int t = l - (63 - __builtin_clzll(lo));
    d = t < d ? t : d;
  }
  const uint64_t hi = m >> l;  // bits l .. 63, bit l first
  if (hi) {
    const int t = __builtin_ctzll(hi);
    d = t < d ? t : d;
  }
  return d < sat ? d : sat;
}

// min over dj in [-lo, hi] of g[dj * stride]^2 + dj^2, or `start` (cap2 + 1) if none is below it.  g points at the cell's own
// column of pass 1; lo / hi: how far the row reaches before / behind it (min(R, columns that exist)).  steps (host tests):
// the number of g read.  The walk ends at the first dj with dj^2 >= best: no g^2 + dj^2 from there on is below best.
template <class G>
TE_DIST_HD uint32_t row_min(const G* g, ptrdiff_t stride, int lo, int hi, uint32_t start, int* steps = nullptr) {
  uint32_t best = start;
  {
    const uint32_t v = (uint32_t)g[0];
    if (v * v < best) best = v * v;
    if (steps) ++*steps;
  }
  const int far = lo > hi ? lo : hi;
  for (int dj = 1; dj <= far; ++dj) {
    const uint32_t dd = (uint32_t)dj * (uint32_t)dj;
    if (dd >= best) break;
    if (dj <= lo) {
      const uint32_t v = (uint32_t)g[-(ptrdiff_t)dj * stride], s = v * v + dd;
      if (s < best) best = s;
      if (steps) ++*steps;
    }
    if (dj <= hi) {
      const uint32_t v = (uint32_t)g[(ptrdiff_t)dj * stride], s = v * v + dd;
      if (s < best) best = s;
      if (steps) ++*steps;
    }
  }
  return best;
}

// the output of a cell: a seed has d2 = 0 and gets 0.0f
TE_DIST_HD float value_of(uint32_t d2, uint32_t cap2, double res, float beyond) { return d2 <= cap2 ? (float)(sqrt((double)d2) * res) : beyond; }

}  // namespace distance
}  // namespace te
