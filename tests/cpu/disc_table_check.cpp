// te_disc_table.h on the CPU (tests/test_filter_table.py).
//   disc_table_check RADIUS RES   the table: "R reach npoints n_ties", the half-widths, the tie offsets (di dj ...)
//   disc_table_check sweep        the table against build_disc (te_disc.h, the function the library ships) for every radius
//                                 build_disc accepts in a sweep; prints "checked mismatches"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "te_disc.h"
#include "te_disc_table.h"

using te::Disc;
using te::kMaxRadiusCells;

namespace {

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
          if (te::build_disc(radius, res, &d) != te::kDiscOk) continue;
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
