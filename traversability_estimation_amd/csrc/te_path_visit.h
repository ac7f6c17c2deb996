// te_path_visit.h -- the plan of the on-demand circular path check (te_check_footprint_paths_radius; kernels in
// te_path_discs.hip, host driver in te_paths_api.hip).
//
// checkCircularFootprintPath (TraversabilityMap.cpp:345-462) calls isTraversable(centre, radius + offset, .., radius) at the
// centres a path visits and nowhere else: the single pose of a one-pose path (:365-385), or, for every segment, the cells of a
// LineIterator from the END index to the START index, the first and then every fourth (nSkip = 3, :396-441).  This header
// holds that enumeration (visit_path), its size without the walk (count_path_visits), the radius classes of a request
// (class_radii) and the 64-bit key (radius class, cell) under which a disc is evaluated once per call (pack_key).
//
// The enumeration depends on the geometry alone: it does not stop at an unsafe centre (the reference does; the batched form
// evaluates every visited centre, the results are the same) and knows nothing of checkInclination.  It stops where the
// reference's own walk has no defined continuation: a segment with an end outside the map (status 1).
//
// G is the geometry: inside(x, y), to_index(x, y, i, j) and a nested Line (init / past_end / next / i / j).  The kernels pass
// te_geom.h's functions and its LineIt; Geom below is the same arithmetic in plain C++ for the host driver's sizing and for
// the CPU check tests/cpu/path_visit_check.cpp, which compiles this text with the host compiler.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define TE_PV_HD __host__ __device__ __forceinline__
#else
#define TE_PV_HD inline
#endif

namespace te {
namespace pv {

constexpr int kSkip = 3;                   // nSkip :396
constexpr int kCellBits = 48;              // key = class << 48 | (j * rows + i)
constexpr int kMaxClasses = 1 << 16;       // distinct radii of one call
constexpr uint64_t kEmptyKey = ~(uint64_t)0;  // (class 65535 with cell 2^48 - 1: no map has that cell)

TE_PV_HD uint64_t pack_key(unsigned cls, int i, int j, int rows) {
  return ((uint64_t)cls << kCellBits) | ((uint64_t)j * (uint64_t)rows + (uint64_t)i);
}
TE_PV_HD unsigned key_class(uint64_t key) { return (unsigned)(key >> kCellBits); }
TE_PV_HD uint64_t key_cell(uint64_t key) { return key & (((uint64_t)1 << kCellBits) - 1); }
// slot of a key in an open-addressing table of 2^k entries (the finaliser of MurmurHash3: every input bit reaches the low bits)
TE_PV_HD uint64_t hash_key(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}
// entries of the table for n_visits insertions: a power of two, at most half full
inline uint64_t table_entries(uint64_t n_visits) {
  uint64_t cap = 64;
  while (cap < 2 * n_visits) cap <<= 1;
  return cap;
}

// grid_map_core's geometry in plain C++ (te_geom.h: the same expressions on the device)
struct Geom {
  int rows, cols;
  double res, len_x, len_y, pos_x, pos_y;
  bool inside(double x, double y) const {  // checkIfPositionWithinMap
    const double tx = -((x - pos_x) - 0.5 * len_x);
    const double ty = -((y - pos_y) - 0.5 * len_y);
    return tx >= 0.0 && ty >= 0.0 && tx < len_x && ty < len_y;
  }
  bool to_index(double x, double y, int& i, int& j) const {  // getIndexFromPosition
    const double vx = ((x - 0.5 * len_x) - pos_x) / res;
    const double vy = ((y - 0.5 * len_y) - pos_y) / res;
    // (a position far outside: the cast is defined only within int's range, and the result is false either way)
    i = (fabs(vx) < 2e9) ? (int)(-vx) : -1;
    j = (fabs(vy) < 2e9) ? (int)(-vy) : -1;
    return inside(x, y) && i >= 0 && j >= 0 && i < rows && j < cols;
  }
  struct Line {  // grid_map::LineIterator
    int i, j, inc1i, inc1j, inc2i, inc2j, den, num, numadd, ncells, icell;
    void init(int si, int sj, int ei, int ej) {
      icell = 0;
      i = si;
      j = sj;
      const int dx = ei > si ? ei - si : si - ei, dy = ej > sj ? ej - sj : sj - ej;
      inc1i = inc2i = (ei >= si) ? 1 : -1;
      inc1j = inc2j = (ej >= sj) ? 1 : -1;
      if (dx >= dy) {
        inc1i = 0;
        inc2j = 0;
        den = dx;
        num = dx / 2;
        numadd = dy;
        ncells = dx + 1;
      } else {
        inc2i = 0;
        inc1j = 0;
        den = dy;
        num = dy / 2;
        numadd = dx;
        ncells = dy + 1;
      }
    }
    bool past_end() const { return icell >= ncells; }
    void next() {
      num += numadd;
      if (num >= den) {
        num -= den;
        i += inc1i;
        j += inc1j;
      }
      i += inc2i;
      j += inc2j;
      icell++;
    }
  };
};

// The centres of one path, in the reference's order; emit(i, j) for each.  Returns the status the geometry gives the
// path: 0, 1 (a segment with an end outside the map: the walk ends before it) or 2 (no poses, :330-334).
// A one-pose path whose pose lies outside the map visits no centre (its value is traversabilityDefault_, :662-664).
template <class G, class F>
TE_PV_HD int visit_path(const G& g, int n, const double* xy, F&& emit) {
  if (n <= 0) return 2;
  if (n == 1) {
    int ci, cj;
    if (g.to_index(xy[0], xy[1], ci, cj)) emit(ci, cj);
    return 0;
  }
  for (int p = 1; p < n; ++p) {
    int si, sj, ei, ej;
    if (!g.to_index(xy[2 * (p - 1)], xy[2 * (p - 1) + 1], si, sj) || !g.to_index(xy[2 * p], xy[2 * p + 1], ei, ej)) return 1;
    typename G::Line L;
    for (L.init(ei, ej, si, sj); !L.past_end(); L.next()) {  // from the end index to the start index
      emit(L.i, L.j);
      for (int s = 0; s < kSkip; ++s)
        if (!L.past_end()) L.next();
    }
  }
  return 0;
}

// the number of centres visit_path emits, without walking the lines: a line of c cells gives ceil(c / 4)
template <class G>
TE_PV_HD long long count_path_visits(const G& g, int n, const double* xy) {
  if (n <= 0) return 0;
  int si, sj, ei, ej;
  if (n == 1) return g.to_index(xy[0], xy[1], si, sj) ? 1 : 0;
  long long total = 0;
  for (int p = 1; p < n; ++p) {
    if (!g.to_index(xy[2 * (p - 1)], xy[2 * (p - 1) + 1], si, sj) || !g.to_index(xy[2 * p], xy[2 * p + 1], ei, ej)) break;
    const int dx = ei > si ? ei - si : si - ei, dy = ej > sj ? ej - sj : sj - ej;
    total += ((dx > dy ? dx : dy) + 1 + kSkip) / (kSkip + 1);
  }
  return total;
}

// Radius classes of a request: uniq = the distinct radii in ascending order, cls[k] = the index of radius[k] in it.
// (-0.0 and 0.0 are one class.)  The radii are finite (the caller checked).
inline void class_radii(int n, const double* radius, std::vector<double>* uniq, std::vector<int>* cls) {
  uniq->assign(radius, radius + n);
  std::sort(uniq->begin(), uniq->end());
  uniq->erase(std::unique(uniq->begin(), uniq->end()), uniq->end());
  cls->resize((size_t)n);
  for (int k = 0; k < n; ++k) (*cls)[k] = (int)(std::lower_bound(uniq->begin(), uniq->end(), radius[k]) - uniq->begin());
}

}  // namespace pv
}  // namespace te
