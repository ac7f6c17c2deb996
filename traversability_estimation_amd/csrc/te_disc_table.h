// te_disc_table.h -- host table of a filter disc of any radius (te_filter_any.hip).
//
// The disc {(di, dj): di^2 + dj^2 <= (radius / res)^2} of the normals, roughness and step windows, in the form build_disc
// (te_disc.h) gives it, without its bounds (kMaxRadiusCells rows, kMaxTies offsets on the circle):
//   - the row runs: column offset dj (|dj| <= R) holds di in [-hw[|dj|], hw[|dj|]];
//   - the tie offsets: squared norm equal to (radius / res)^2 to within 1e-9 relative; CircleIterator decides them per
//     centre from rounded double positions, the kernels with the same formula -- any number of them;
//   - R, reach (largest |di| or |dj| of runs and ties) and npoints (cells of the runs).
// For every radius build_disc accepts the table is the same disc: tests/cpu/disc_table_check.cpp.
// Plain C++ (no HIP): the library and the CPU check compile the same text.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

namespace te {

struct DiscTable {
  double r2 = 0.0;            // radius * radius (double, as CircleIterator computes it)
  int R = -1;                 // largest |dj| of the runs; -1: no run
  int reach = 0;              // max(R, hw[0], largest |offset| of a tie)
  long long npoints = 0;      // cells of the runs
  std::vector<int32_t> hw;    // [0 .. R], non-increasing
  std::vector<int32_t> ties;  // (di, dj) pairs, in build_disc's order
  int n_ties() const { return (int)ties.size() / 2; }
};

// the table of the disc of `radius` on a map of resolution `res`: build_disc's classification, O(radius) offsets looked at
inline void build_disc_table(double radius, double res, DiscTable* t) {
  t->r2 = radius * radius;
  t->hw.clear();
  t->ties.clear();
  t->R = -1;
  t->reach = 0;
  t->npoints = 0;
  const double q = (radius / res) * (radius / res);
  const double tol = 1e-9 * (q > 1.0 ? q : 1.0);
  const double rmax = sqrt(q + tol);
  const int lim = (int)floor(rmax) + 1;
  std::vector<int32_t> hw((size_t)lim + 1, -1);
  for (int b = 0; b <= lim; ++b) {
    // only the offsets around the end of the run can be ties or outside: a <= s - 3 with s = sqrt(q + tol - b^2) has
    // a^2 + b^2 <= q + tol - 6 s + 9 < q - tol (s >= 3, tol < 4.5)
    const double s = sqrt(fmax(q + tol - (double)b * b, 0.0));
    long long a_hi = (long long)floor(s) + 1;
    if (a_hi > lim) a_hi = lim;
    const long long a_lo = a_hi - 3 < 0 ? 0 : a_hi - 3;
    int h = (int)a_lo - 1;
    for (long long a = a_lo; a <= a_hi; ++a) {
      const double m = (double)(a * a + (long long)b * b);
      if (fabs(m - q) <= tol) {  // tie: all sign combinations, each listed once
        for (int sa = -1; sa <= 1; sa += 2)
          for (int sb = -1; sb <= 1; sb += 2) {
            if ((a == 0 && sa < 0) || (b == 0 && sb < 0)) continue;
            t->ties.push_back((int32_t)(sa * a));
            t->ties.push_back((int32_t)(sb * b));
            const int mx = (int)(a > b ? a : b);
            if (mx > t->reach) t->reach = mx;
          }
      } else if (m < q) {
        h = (int)a;
      }
    }
    hw[b] = h;
    if (h >= 0) {
      t->R = b;
      t->npoints += (b == 0 ? 1 : 2) * (2 * (long long)h + 1);
    }
  }
  t->hw.assign(hw.begin(), hw.begin() + (t->R + 1));
  if (t->R > t->reach) t->reach = t->R;
  if (t->R >= 0 && t->hw[0] > t->reach) t->reach = t->hw[0];
}

// same_disc (te_disc.h) for tables: the same cells, and the same per-centre test of the ties
inline bool same_disc_table(const DiscTable& a, const DiscTable& b) {
  if (a.R != b.R || a.hw != b.hw || a.ties.size() != b.ties.size()) return false;
  if (!a.ties.empty() && a.r2 != b.r2) return false;
  for (size_t k = 0; k < a.ties.size(); k += 2) {  // (the same set)
    bool found = false;
    for (size_t l = 0; l < b.ties.size() && !found; l += 2) found = a.ties[k] == b.ties[l] && a.ties[k + 1] == b.ties[l + 1];
    if (!found) return false;
  }
  return true;
}

}  // namespace te
