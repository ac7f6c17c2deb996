// CPU check of the submap plan (traversability_estimation_amd/csrc/te_submap_plan.h), the geometry te_submap_geometry hands out
// and te_download_submap's kernel indexes memory with.  tests/test_submap_plan.py compares the plan with the independent
// restatement (tests/ref_py/grid_map_ref.py) bit for bit; this program checks, on the header alone and under the sanitizers,
// what must hold whatever the arithmetic's last bit is.  For every request:
//   - arguments no request can have are refused before anything is computed, and leave a zeroed plan;
//   - ok = 0 leaves a zeroed plan;
//   - ok = 1: the rectangle lies in the map and has at least one cell -- what the kernel relies on --, the submap's length is
//     size * resolution exactly, its centre is the middle of the rectangle's outer corners (to a few ulps of the coordinates),
//     the requested centre lies in the submap, and each outer row / column holds the clamped requested corner;
//   - a centre well inside the map is ok, a centre outside the map is not.
// Named cases: the whole map, a request larger than the map, zero length, the centre on each border, the far corner cell.
//   submap_plan_check [n_random seed]
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>
#include <limits>

#include "te_submap_plan.h"

namespace {

int g_failed = 0, g_ok = 0, g_not_ok = 0;
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

struct Map {
  int rows, cols;
  double res, px, py;
};

bool zeroed(const te_submap_info& s) {
  const te_submap_info z = te_submap_info();
  return s.ok == 0 && s.row0 == z.row0 && s.col0 == 0 && s.rows == 0 && s.cols == 0 && s.pos_x == 0.0 && s.pos_y == 0.0 && s.length_x == 0.0 &&
         s.length_y == 0.0;
}

te_submap_info request(const Map& m, double x, double y, double lx, double ly, int expect_rc = TE_OK) {
  te_submap_info s;
  memset(&s, 0x5a, sizeof(s));
  const char* why = nullptr;
  const int rc = te::submap::plan(m.rows, m.cols, m.res, m.px, m.py, x, y, lx, ly, &s, &why);
  CHECK(rc == expect_rc, "%dx%d: rc %d for (%g, %g) + (%g, %g)", m.rows, m.cols, rc, x, y, lx, ly);
  if (rc != TE_OK) CHECK(zeroed(s) && why && why[0], "%dx%d: a refused request leaves a zeroed plan and a reason", m.rows, m.cols);
  return s;
}

// one axis of an ok plan: n cells of the map around `mp`, the request c + l, the plan's first cell i0, size k, position sp, length sl
void check_axis(const char* name, int n, double res, double mp, double c, double l, int i0, int k, double sp, double sl) {
  const double len = n * res, top = mp + 0.5 * len;  // the map's upper border: index 0 starts there, indices grow downwards
  const double tol = 64.0 * 2.220446049250313e-16 * (fabs(mp) + len + fabs(c) + l + 1.0);
  CHECK(i0 >= 0 && k >= 1 && k <= n - i0, "%s: cells [%d, %d) of %d", name, i0, i0 + k, n);
  CHECK(sl == k * res, "%s: length %.17g for %d cells", name, sl, k);
  const double hi = top - i0 * res, lo = top - (i0 + k) * res;  // the rectangle's outer corners
  CHECK(fabs(sp - 0.5 * (hi + lo)) <= tol, "%s: position %.17g, the rectangle's middle is %.17g", name, sp, 0.5 * (hi + lo));
  CHECK(c <= hi + tol && c >= lo - tol, "%s: the centre %.17g outside [%.17g, %.17g]", name, c, lo, hi);
  // the clamped corners lie in the first and in the last cell
  const double up = fmin(c + 0.5 * l, top), down = fmax(c - 0.5 * l, top - len);
  CHECK(up <= hi + tol && up >= hi - res - tol, "%s: the upper corner %.17g is not in cell %d", name, up, i0);
  CHECK(down >= lo - tol && down <= lo + res + tol, "%s: the lower corner %.17g is not in cell %d", name, down, i0 + k - 1);
}

void check_request(const Map& m, double x, double y, double lx, double ly) {
  const te_submap_info s = request(m, x, y, lx, ly);
  const double len_x = m.rows * m.res, len_y = m.cols * m.res;
  const double dx = (m.px + 0.5 * len_x) - x, dy = (m.py + 0.5 * len_y) - y;  // distance below the upper borders
  const double margin = 1e-9 * (fabs(m.px) + fabs(m.py) + len_x + len_y + 1.0);
  if (dx > margin && dx < len_x - margin && dy > margin && dy < len_y - margin)
    CHECK(s.ok == 1, "%dx%d: a centre inside the map, (%.17g, %.17g) + (%g, %g), is refused", m.rows, m.cols, x, y, lx, ly);
  if (dx < -margin || dx > len_x + margin || dy < -margin || dy > len_y + margin)
    CHECK(s.ok == 0, "%dx%d: a centre outside the map, (%.17g, %.17g), is served", m.rows, m.cols, x, y);
  if (!s.ok) {
    ++g_not_ok;
    CHECK(zeroed(s), "%dx%d: ok = 0 with a plan", m.rows, m.cols);
    return;
  }
  ++g_ok;
  check_axis("rows", m.rows, m.res, m.px, x, lx, s.row0, s.rows, s.pos_x, s.length_x);
  check_axis("cols", m.cols, m.res, m.py, y, ly, s.col0, s.cols, s.pos_y, s.length_y);
}

void named(const Map& m) {
  const double len_x = m.rows * m.res, len_y = m.cols * m.res;
  // the whole map, and a request larger than the map (clamped)
  for (const double f : {1.0, 1.5, 40.0}) {
    const te_submap_info s = request(m, m.px, m.py, f * len_x, f * len_y);
    CHECK(s.ok == 1 && s.row0 == 0 && s.col0 == 0 && s.rows == m.rows && s.cols == m.cols, "%dx%d x %g: (%d,%d)+(%d,%d)", m.rows, m.cols, f,
          s.row0, s.col0, s.rows, s.cols);
    CHECK(s.length_x == len_x && s.length_y == len_y, "%dx%d x %g: lengths", m.rows, m.cols, f);
    check_request(m, m.px, m.py, f * len_x, f * len_y);
  }
  // zero length: the one cell under the centre -- here the middle of cell (i, j)
  const int cells[][2] = {{0, 0}, {m.rows - 1, m.cols - 1}, {m.rows / 2, m.cols / 3}, {0, m.cols - 1}, {m.rows - 1, 0}};
  for (const auto& c : cells) {
    const double x = m.px + 0.5 * len_x - (c[0] + 0.5) * m.res, y = m.py + 0.5 * len_y - (c[1] + 0.5) * m.res;
    const te_submap_info s = request(m, x, y, 0.0, 0.0);
    CHECK(s.ok == 1 && s.row0 == c[0] && s.col0 == c[1] && s.rows == 1 && s.cols == 1, "%dx%d: zero length at cell (%d,%d): (%d,%d)+(%d,%d)", m.rows,
          m.cols, c[0], c[1], s.row0, s.col0, s.rows, s.cols);
    check_request(m, x, y, 0.0, 0.0);
    // the far corner cell (and the others) with a length that reaches beyond the map on two sides
    check_request(m, x, y, 3.0 * m.res, 5.0 * m.res);
  }
  // the centre exactly on each of the four borders: served or refused, never out of the map (check_request's invariants)
  for (const double lx : {0.0, 2.5 * m.res}) {
    check_request(m, m.px + 0.5 * len_x, m.py, lx, lx);
    check_request(m, m.px - 0.5 * len_x, m.py, lx, lx);
    check_request(m, m.px, m.py + 0.5 * len_y, lx, lx);
    check_request(m, m.px, m.py - 0.5 * len_y, lx, lx);
  }
  // arguments no request can have
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  for (const double bad : {nan, inf, -inf}) {
    request(m, bad, m.py, 1.0, 1.0, TE_ERR_INVALID_ARG);
    request(m, m.px, bad, 1.0, 1.0, TE_ERR_INVALID_ARG);
    request(m, m.px, m.py, bad, 1.0, TE_ERR_INVALID_ARG);
    request(m, m.px, m.py, 1.0, bad, TE_ERR_INVALID_ARG);
  }
  request(m, m.px, m.py, -1e-300, 1.0, TE_ERR_INVALID_ARG);
  request(m, m.px, m.py, 1.0, -2.0, TE_ERR_INVALID_ARG);
  request(m, m.px, m.py, -0.0, 0.0);  // (minus zero is zero)
  // far away, and as far as doubles go: refused as requests, never undefined
  check_request(m, m.px + 1e6, m.py - 1e6, 1.0, 1.0);
  for (const double far : {1e300, -1e300, 1.7e308}) CHECK(request(m, far, m.py, 1.0, 1.7e308).ok == 0, "%dx%d: a request at %g is served", m.rows, m.cols, far);
  Map bad = m;
  bad.rows = 0;
  request(bad, m.px, m.py, 1.0, 1.0, TE_ERR_INVALID_ARG);
  bad = m;
  bad.res = 0.0;
  request(bad, m.px, m.py, 1.0, 1.0, TE_ERR_INVALID_ARG);
  bad = m;
  bad.py = nan;
  request(bad, m.px, m.py, 1.0, 1.0, TE_ERR_INVALID_ARG);
}

uint64_t g_rng = 1;
uint64_t rnd() {  // splitmix64
  uint64_t z = (g_rng += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
double uniform() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }

}  // namespace

int main(int argc, char** argv) {
  const int n_random = argc > 1 ? atoi(argv[1]) : 4000;
  g_rng = argc > 2 ? (uint64_t)atoll(argv[2]) : 1;
  const Map maps[] = {{1, 1, 0.03, 0.0, 0.0},       {7, 5, 0.05, 100.0, -250.3},   {37, 29, 0.1, -3.25, 7.5},
                      {100, 133, 0.03, 100.0, -250.3}, {4096, 4096, 0.03, 12.0, -7.0}, {1, 64, 0.05, 0.0, 1e4}};
  const int n_maps = (int)(sizeof(maps) / sizeof(maps[0]));
  for (const Map& m : maps) named(m);
  const int named_requests = g_ok + g_not_ok;
  g_ok = g_not_ok = 0;
  for (int k = 0; k < n_random; ++k) {
    const Map& m = maps[rnd() % n_maps];
    const double len_x = m.rows * m.res, len_y = m.cols * m.res;
    // centres in the map's extent widened by 10 % on every side, lengths from 0 to 1.5 x the map's
    const double x = m.px + (uniform() - 0.5) * 1.2 * len_x, y = m.py + (uniform() - 0.5) * 1.2 * len_y;
    const double lx = rnd() % 16 == 0 ? 0.0 : uniform() * 1.5 * len_x, ly = rnd() % 16 == 0 ? 0.0 : uniform() * 1.5 * len_y;
    check_request(m, x, y, lx, ly);
  }
  CHECK(n_random < 400 || (2 * g_ok >= n_random && g_not_ok >= 50), "%d of %d random requests ok, %d not", g_ok, n_random, g_not_ok);
  printf("%d named and %d random requests (%d ok), %d failed checks\n", named_requests, n_random, g_ok, g_failed);
  return g_failed ? 1 : 0;
}
