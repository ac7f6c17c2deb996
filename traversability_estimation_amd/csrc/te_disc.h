// te_disc.h -- the host tables the filters and the shape-specialised footprint kernels take their shape from: a disc's row
// runs and tie offsets (build_disc), the disc with the cells on its circle and the circle's packed offsets (build_tie_circle),
// the summary of the ties the footprint route asks for (tie_summary) and the clip table of border moments
// (build_clip_table).  Plain C++ of plain values (no HIP): the library and the CPU checks (tests/cpu/disc_check.cpp,
// disc_table_check.cpp, fp_route_check.cpp) compile the same text.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

namespace te {

constexpr int kMaxRadiusCells = 32;  // largest stencil radius (in cells) a launch supports
constexpr int kMaxTies = 32;         // offsets lying exactly on the circle (tie radii)

// A disc {(di,dj): di^2+dj^2 <= (radius/res)^2} as row runs: for column offset dj (|dj|<=R) the cells
// di in [-hw[|dj|], hw[|dj|]].  Offsets whose squared norm equals (radius/res)^2 up to rounding are
// NOT in the runs: whether CircleIterator keeps them depends on the double rounding of the cell
// positions, so they are listed in `tie_*` and tested per cell with the reference's own formula.
struct Disc {
  int R;                         // largest |offset| in the runs (-1: empty disc)
  int hw[kMaxRadiusCells + 1];   // -1 where the run is empty
  int n_ties;
  int8_t tie_di[kMaxTies], tie_dj[kMaxTies];
  double r2;                     // radius*radius (double, as CircleIterator computes it)
  int reach;                     // max(R, max |tie offset|)
  int npoints;                   // number of cells in the runs (full disc, away from borders)
  int Q;                         // tie-free discs: largest a^2+b^2 <= (radius/res)^2 (names the shape); -1 with ties
  // TE_OPT_FILTER_ANY_RADIUS: a disc the fixed arrays above do not hold (or every disc under option 2) takes the kernels of
  // te_filter_any.hip.  Its runs and ties are in the device table `tab` (te_disc_table.h: hw[0 .. R], then n_ties (di, dj)
  // int32 pairs); hw[] holds -1 and Q is -1, and every other kernel's route refuses the disc.
  int any;
  int any_hw0;                   // (host copy of tab[0]: the widest run)
  const int* tab;
};

enum DiscStatus { kDiscOk = 0, kDiscTooLarge, kDiscTooManyTies };  // (the fixed arrays of Disc hold neither)

// Build the row-run table of the disc {di^2+dj^2 <= (radius/res)^2}.  Offsets whose squared norm
// equals (radius/res)^2 to within 1e-9 relative are "ties": the reference decides them per cell
// from rounded double positions, so the kernels test them with the same formula.
inline DiscStatus build_disc(double radius, double res, Disc* d) {
  memset(d, 0, sizeof(*d));
  d->r2 = radius * radius;
  const double q = (radius / res) * (radius / res);
  const double tol = 1e-9 * (q > 1.0 ? q : 1.0);
  const double rmax = sqrt(q + tol);
  if (!(rmax < (double)kMaxRadiusCells + 0.5)) return kDiscTooLarge;
  const int lim = (int)floor(rmax) + 1;
  d->R = -1;
  d->reach = 0;
  d->npoints = 0;
  for (int b = 0; b <= kMaxRadiusCells; ++b) d->hw[b] = -1;
  for (int b = 0; b <= lim && b <= kMaxRadiusCells; ++b) {
    int hw = -1;
    for (int a = 0; a <= lim; ++a) {
      const double m = (double)(a * a + b * b);
      if (fabs(m - q) <= tol) {
        // tie: all sign combinations, each listed once
        for (int sa = -1; sa <= 1; sa += 2)
          for (int sb = -1; sb <= 1; sb += 2) {
            if ((a == 0 && sa < 0) || (b == 0 && sb < 0)) continue;
            if (d->n_ties >= kMaxTies) return kDiscTooManyTies;
            d->tie_di[d->n_ties] = (int8_t)(sa * a);
            d->tie_dj[d->n_ties] = (int8_t)(sb * b);
            d->n_ties++;
            const int mx = a > b ? a : b;
            if (mx > d->reach) d->reach = mx;
          }
      } else if (m < q) {
        hw = a;
      }
    }
    d->hw[b] = hw;
    if (hw >= 0) {
      d->R = b;
      d->npoints += (b == 0 ? 1 : 2) * (2 * hw + 1);
    }
  }
  // rows are nested (hw non-increasing) and a tie at (a,b) always sits right after the run end, so
  // runs never skip an interior cell.
  if (d->R > d->reach) d->reach = d->R;
  if (d->hw[0] > d->reach) d->reach = d->hw[0];
  // the shape is named by the largest sum of two squares not above q (only meaningful without ties)
  d->Q = -1;
  if (d->n_ties == 0) {
    int best = -1;
    for (int a = 0; a <= lim; ++a)
      for (int b = 0; b <= lim; ++b) {
        const int m = a * a + b * b;
        if ((double)m < q && m > best) best = m;
      }
    d->Q = best;  // -1: radius below zero cells cannot happen (m = 0 < q unless q == 0, which is a tie)
  }
  return kDiscOk;
}

inline bool same_disc(const Disc& a, const Disc& b) {
  if (a.R != b.R || a.n_ties != b.n_ties) return false;
  for (int k = 0; k <= kMaxRadiusCells; ++k)
    if (a.hw[k] != b.hw[k]) return false;
  if (a.n_ties && a.r2 != b.r2) return false;
  return true;
}

// A tie radius for the sliding kernels (te_normals3.hip: TIES march, te_footprint4.hip): the disc WITH the cells on its
// circle, and the circle's offsets with both parts non-zero, packed, in tie order (the kernels handle (+-R, 0) and
// (0, +-R) themselves).
struct TieCircle {
  Disc full;
  int gen[kMaxTies], n_gen;
};
inline void build_tie_circle(const Disc& d, TieCircle* c) {
  c->full = d;
  c->n_gen = 0;
  for (int t = 0; t < d.n_ties; ++t) {
    const int ai = abs((int)d.tie_di[t]), aj = abs((int)d.tie_dj[t]);
    if (c->full.hw[aj] < ai) c->full.hw[aj] = ai;
    if (c->full.R < aj) c->full.R = aj;
    if (ai != 0 && aj != 0) c->gen[c->n_gen++] = ((int)d.tie_di[t] & 0xff) | (((int)d.tie_dj[t] & 0xff) << 8);
  }
}

// What plan_fp_route (te_fp_route.h) asks about the ties of a footprint disc of the given reach: whether every tie offset
// has the squared norm reach^2 (a whole-cell radius), and how many have both parts non-zero.
inline void tie_summary(const Disc& d, int reach, bool* on_circle, int* n_gen) {
  *on_circle = true;
  *n_gen = 0;
  for (int t = 0; t < d.n_ties; ++t) {
    *on_circle = *on_circle && (int)d.tie_di[t] * d.tie_di[t] + (int)d.tie_dj[t] * d.tie_dj[t] == reach * reach;
    *n_gen += (d.tie_di[t] != 0 && d.tie_dj[t] != 0) ? 1 : 0;
  }
}

// What plan_chain_route (te_chain_route.h) asks about a filter's disc, plain values (O(R) to fill)
struct DiscSummary {
  bool any = false;  // Disc::any: the kernels of te_filter_any.hip, nothing else below is meaningful
  int R = -1, Q = -1, reach = 0, npoints = 0, n_ties = 0;
  bool ties_on_circle = true;  // every tie offset has the squared norm reach^2 (a whole-cell radius)
  int n_gen = 0;               // tie offsets with both parts non-zero
  int q_runs = 0;              // largest di^2 + dj^2 in the runs: the shape a tie disc leaves without its circle
  int n_offsets = 0;           // cells besides the centre, runs and ties together
  long long sii_runs = 0, sii_ties = 0;  // sum of di^2 over the runs / over the tie offsets
};
inline DiscSummary disc_summary(const Disc& d) {
  DiscSummary s;
  s.any = d.any != 0;
  s.R = d.R;
  s.Q = d.Q;
  s.reach = d.reach;
  s.npoints = d.npoints;
  s.n_ties = d.n_ties;
  if (s.any) return s;
  tie_summary(d, d.reach, &s.ties_on_circle, &s.n_gen);
  for (int b = 0; b <= d.R; ++b) {
    const int hw = d.hw[b];
    if (hw < 0) continue;
    if (hw * hw + b * b > s.q_runs) s.q_runs = hw * hw + b * b;
    s.sii_runs += (b == 0 ? 1 : 2) * ((long long)hw * (hw + 1) * (2 * hw + 1) / 3);
  }
  s.n_offsets = d.npoints > 0 ? d.npoints - 1 : 0;
  for (int t = 0; t < d.n_ties; ++t) {
    s.sii_ties += (int)d.tie_di[t] * d.tie_di[t];
    s.n_offsets += (d.tie_di[t] != 0 || d.tie_dj[t] != 0) ? 1 : 0;
  }
  return s;
}

// x/y moments of the disc clipped to di in [lo_i, hi_i], dj in [lo_j, hi_j] for every clip code (kx, ky) in [-R, R]^2
// (see k_normals_slide): n, sum di, sum dj, sum di^2, sum di dj, sum dj^2.  out must hold (2R+1)^2 * 6 ints.
inline void build_clip_table(const Disc& d, int R, int* out) {
  for (int ky = -R; ky <= R; ++ky)
    for (int kx = -R; kx <= R; ++kx) {
      const int lo_i = kx > 0 ? -R + kx : -R, hi_i = kx < 0 ? R + kx : R;
      const int lo_j = ky > 0 ? -R + ky : -R, hi_j = ky < 0 ? R + ky : R;
      int n = 0, si = 0, sj = 0, sii = 0, sij = 0, sjj = 0;
      for (int dj = lo_j; dj <= hi_j; ++dj) {
        const int adj = dj < 0 ? -dj : dj;
        const int hw = adj <= d.R ? d.hw[adj] : -1;
        for (int di = -hw; di <= hw; ++di) {
          if (di < lo_i || di > hi_i) continue;
          ++n;
          si += di;
          sj += dj;
          sii += di * di;
          sij += di * dj;
          sjj += dj * dj;
        }
      }
      int* e = out + ((ky + R) * (2 * R + 1) + (kx + R)) * 6;
      e[0] = n; e[1] = si; e[2] = sj; e[3] = sii; e[4] = sij; e[5] = sjj;
    }
}

}  // namespace te
