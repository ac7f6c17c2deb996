// CPU check of the median-fill plan (traversability_estimation_amd/csrc/te_median_plan.h), the header te_run_median_fill's
// launcher takes every size from.  tests/test_median_plan.py runs it plain and under the sanitizers.
//   median_plan_check                               the invariants below over a sweep of shapes and radii
//   median_plan_check radius RADIUS RESOLUTION      prints (size_t)(radius / resolution)
//   median_plan_check route ROWS COLS NMAPS R OPT   prints "tile|any r lds_bytes blocks tiles_x tiles_y"
// Invariants: the tile route is taken exactly when the staged rectangle and the list fit the LDS budget (and never under
// option 2); its LDS bytes are those of (64 + 2r) x (16 + 2r) keys and 1024 list entries; the tiles cover the map and no tile
// lies outside it; the clamped radius is the quotient cut at the map's longer side; every map takes one of the two routes.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "te_median_plan.h"

using namespace te::median;

namespace {
int g_failed = 0;
#define CHECK(cond, ...)              \
  do {                                \
    if (!(cond)) {                    \
      ++g_failed;                     \
      if (g_failed <= 20) {           \
        printf("FAILED %s: ", #cond); \
        printf(__VA_ARGS__);          \
        printf("\n");                 \
      }                               \
    }                                 \
  } while (0)
}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "radius")) {
    printf("%llu\n", radius_cells_unclamped(atof(argv[2]), atof(argv[3])));
    return 0;
  }
  if (argc == 7 && !strcmp(argv[1], "route")) {
    const Plan p = plan(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]));
    printf("%s %d %zu %zu %d %d\n", p.route == kRouteTile ? "tile" : "any", p.r, p.lds_bytes, p.blocks, p.tiles_x, p.tiles_y);
    return 0;
  }
  int n = 0;
  const int shapes[][2] = {{1, 1}, {5, 7}, {64, 16}, {65, 17}, {70, 37}, {130, 33}, {96, 80}, {200, 128}, {4096, 4096}, {1, 100000}, {100000, 1}};
  for (const auto& s : shapes)
    for (int nmaps : {1, 3, 512})
      for (int r = 0; r <= 200; ++r)
        for (int opt = 0; opt <= 2; ++opt) {
          const Plan p = plan(s[0], s[1], nmaps, r, opt);
          ++n;
          const size_t want_lds = (size_t)(64 + 2 * r) * (size_t)(16 + 2 * r) * 4 + 2048;
          const bool fits = want_lds + 64 <= kLdsBudget;  // (64: the kernel's static LDS)
          CHECK(p.route == kRouteTile || p.route == kRouteAny, "route %d", p.route);
          CHECK((p.route == kRouteTile) == (fits && opt != 2), "%dx%d r=%d opt=%d: route %d", s[0], s[1], r, opt, p.route);
          CHECK(p.lds_bytes == (p.route == kRouteTile ? want_lds : 0), "lds %zu", p.lds_bytes);
          CHECK(p.r == r, "r");
          CHECK((long long)p.tiles_x * kTileRows >= s[0] && (long long)(p.tiles_x - 1) * kTileRows < s[0], "tiles_x %d of %d rows", p.tiles_x, s[0]);
          CHECK((long long)p.tiles_y * kTileCols >= s[1] && (long long)(p.tiles_y - 1) * kTileCols < s[1], "tiles_y %d of %d cols", p.tiles_y, s[1]);
          CHECK(p.blocks == (size_t)p.tiles_x * p.tiles_y * nmaps, "blocks");
        }
  CHECK(tile_fits(15) && !tile_fits(16), "the budget admits r <= 15");
  CHECK(!tile_fits(-1), "negative halo");
  // the radius: truncation without a rounding fix, and the cut at the map's longer side
  CHECK(radius_cells_unclamped(0.15, 0.05) == 2, "0.15 / 0.05");
  CHECK(radius_cells_unclamped(0.11, 0.03) == 3, "0.11 / 0.03");
  CHECK(radius_cells_unclamped(0.04, 0.05) == 0, "radius < res");
  CHECK(radius_cells_unclamped(0.0, 0.05) == 0, "0");
  CHECK(radius_cells(0.15, 0.05, 100, 50) == 2, "clamped 0.15 / 0.05");
  CHECK(radius_cells(1e300, 1e-300, 100, 50) == 100, "inf quotient");
  CHECK(radius_cells(7.0, 0.05, 100, 50) == 100, "beyond the map");
  CHECK(radius_cells(4.96, 0.05, 100, 50) == 99, "just inside");
  CHECK(radius_cells(2.0, 0.05, 96, 80) == 40, "2.0 / 0.05");
  printf("%d plans, %d failed checks\n", n, g_failed);
  return g_failed ? 1 : 0;
}
