// te_disc_table.h on the CPU (tests/test_filter_table.py).
//   disc_table_check RADIUS RES   the table: "R reach npoints n_ties", the half-widths, the tie offsets (di dj ...)
//   disc_table_check sweep        the table against build_disc (transcribed below from te_shim.hip, which needs HIP to
//                                 compile) for every radius build_disc accepts in a sweep; prints "checked mismatches"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "te_disc_table.h"

namespace {

constexpr int kMaxRadiusCells = 32;
constexpr int kMaxTies = 32;

struct Disc {
  int R;
  int hw[kMaxRadiusCells + 1];
  int n_ties;
  int tie_di[kMaxTies], tie_dj[kMaxTies];
  double r2;
  int reach;
  int npoints;
};

// te_shim.hip: build_disc (false where it returns TE_ERR_UNSUPPORTED)
bool build_disc(double radius, double res, Disc* d) {
  memset(d, 0, sizeof(*d));
  d->r2 = radius * radius;
  const double q = (radius / res) * (radius / res);
  const double tol = 1e-9 * (q > 1.0 ? q : 1.0);
  const double rmax = sqrt(q + tol);
  if (!(rmax < (double)kMaxRadiusCells + 0.5)) return false;
  const int lim = (int)floor(rmax) + 1;
  d->R = -1;
  for (int b = 0; b <= kMaxRadiusCells; ++b) d->hw[b] = -1;
  for (int b = 0; b <= lim && b <= kMaxRadiusCells; ++b) {
    int hw = -1;
    for (int a = 0; a <= lim; ++a) {
      const double m = (double)(a * a + b * b);
      if (fabs(m - q) <= tol) {
        for (int sa = -1; sa <= 1; sa += 2)
          for (int sb = -1; sb <= 1; sb += 2) {
            if ((a == 0 && sa < 0) || (b == 0 && sb < 0)) continue;
            if (d->n_ties >= kMaxTies) return false;
            d->tie_di[d->n_ties] = sa * a;
            d->tie_dj[d->n_ties] = sb * b;
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
  if (d->R > d->reach) d->reach = d->R;
  if (d->hw[0] > d->reach) d->reach = d->hw[0];
  return true;
}

bool agrees(const Disc& d, const te::DiscTable& t) {
  if (d.R != t.R || d.reach != t.reach || d.npoints != t.npoints || d.n_ties != t.n_ties() || d.r2 != t.r2) return false;
  for (int b = 0; b <= kMaxRadiusCells; ++b)
    if (d.hw[b] != (b <= t.R ? t.hw[b] : -1)) return false;
  for (int k = 0; k < d.n_ties; ++k)  // (the same order, hence the same set)
    if (d.tie_di[k] != t.ties[2 * k] || d.tie_dj[k] != t.ties[2 * k + 1]) return false;
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "sweep")) {
    long checked = 0, bad = 0;
    const double res_list[] = {0.01, 0.02, 0.025, 0.03, 0.05, 0.07, 0.1};
    for (double res : res_list) {
      // fine steps in cells, whole cells, and radii given in metres as a YAML would (0.001 m steps)
      for (int k = 0; k <= 33 * 40; ++k) {
        const double radii[3] = {k / 40.0 * res, (double)(k / 40) * res, k * 0.001};
        for (double radius : radii) {
          Disc d;
          if (!build_disc(radius, res, &d)) continue;
          te::DiscTable t;
          te::build_disc_table(radius, res, &t);
          ++checked;
          if (!agrees(d, t)) {
            if (bad < 10) fprintf(stderr, "mismatch: radius %.17g res %.17g\n", radius, res);
            ++bad;
          }
        }
      }
    }
    printf("%ld %ld\n", checked, bad);
    return 0;
  }
  if (argc != 3) {
    fprintf(stderr, "usage: %s RADIUS RES | sweep\n", argv[0]);
    return 2;
  }
  te::DiscTable t;
  te::build_disc_table(atof(argv[1]), atof(argv[2]), &t);
  printf("%d %d %lld %d\n", t.R, t.reach, t.npoints, t.n_ties());
  for (int v : t.hw) printf("%d ", v);
  printf("\n");
  for (int v : t.ties) printf("%d ", v);
  printf("\n");
  return 0;
}
