// CPU check of the radius-filter plan (traversability_estimation_amd/csrc/te_radius_plan.h): the predicate under which the
// sliding Mean may add in another order, and the route a call takes.  tests/test_radius_plan.py runs it plain and under the
// sanitizers.
//   radius_plan_check                                     the checks below
//   radius_plan_check route OP ROWS COLS RADIUS RES OPT   prints "slide|gather lds_bytes seg levels log2n R hw0 reach n_ties npoints"
//   radius_plan_check free EMAX EMIN LOG2N                prints order_free as 0 / 1
// Checks: for exponent windows exactly at the predicate's limit the sums of random floats in forward, reverse, random and
// column-prefix order all equal the exact sum held in __int128 fixed point; one constructed window just beyond the limit where
// two orders differ; the decision at the LDS limit and at the grid limit; the bounded radius.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "te_disc_table.h"
#include "te_radius_plan.h"

using namespace te::radius;

namespace {
int g_failed = 0, g_checks = 0;
#define CHECK(cond, ...)              \
  do {                                \
    ++g_checks;                       \
    if (!(cond)) {                    \
      ++g_failed;                     \
      if (g_failed <= 20) {           \
        printf("FAILED %s: ", #cond); \
        printf(__VA_ARGS__);          \
        printf("\n");                 \
      }                               \
    }                                 \
  } while (0)

float from_bits(uint32_t b) {
  float f;
  memcpy(&f, &b, sizeof(f));
  return f;
}
uint32_t to_bits(float f) {
  uint32_t b;
  memcpy(&b, &f, sizeof(b));
  return b;
}
uint64_t dbits(double d) {
  uint64_t b;
  memcpy(&b, &d, sizeof(b));
  return b;
}

// a float of binary exponent e (denormal for e = -126 and a mantissa below 2^23), mantissa m < 2^24: m * 2^(e - 23)
float make(int e, uint32_t m, bool neg) {
  uint32_t b;
  if (m < (1u << 23))
    b = m;  // denormal (e = -126)
  else
    b = ((uint32_t)(e + 127) << 23) | (m & 0x7fffffu);
  return from_bits(b | (neg ? 0x80000000u : 0u));
}

// the exact sum in units of 2^(emin - 23)
__int128 exact_units(const std::vector<float>& v, int emin) {
  __int128 s = 0;
  for (float f : v) {
    const uint32_t b = to_bits(f);
    if ((b & 0x7fffffffu) == 0) continue;
    const int e = float_exponent(b);
    const uint32_t m = (b & 0x7fffffu) | (((b >> 23) & 0xffu) ? (1u << 23) : 0u);
    const __int128 t = (__int128)m << (e - emin);
    s += (b >> 31) ? -t : t;
  }
  return s;
}

double sum_in(const std::vector<float>& v, const std::vector<int>& order) {
  double s = 0.0;
  for (int k : order) s += (double)v[(size_t)k];
  return s;
}

// the sliding kernel's order: the values as `cols` column segments, a prefix sum per segment, one run per column as a
// difference of two prefixes, the runs added over the columns; the cells outside the runs are added as "ties" at the end
double sum_prefix(const std::vector<float>& v, int cols, std::mt19937& rng) {
  const int n = (int)v.size(), seg = (n + cols - 1) / cols;
  double total = 0.0;
  std::vector<int> rest;
  for (int c = 0; c < cols; ++c) {
    const int a = c * seg, b = std::min(n, a + seg);
    if (a >= b) break;
    std::vector<double> P((size_t)(b - a) + 1, 0.0);
    for (int t = a; t < b; ++t) P[(size_t)(t - a) + 1] = P[(size_t)(t - a)] + (double)v[(size_t)t];
    int lo = (int)(rng() % (unsigned)(b - a)), hi = (int)(rng() % (unsigned)(b - a));
    if (lo > hi) std::swap(lo, hi);
    total += P[(size_t)hi + 1] - P[(size_t)lo];
    for (int t = a; t < a + lo; ++t) rest.push_back(t);
    for (int t = a + hi + 1; t < b; ++t) rest.push_back(t);
  }
  for (int t : rest) total += (double)v[(size_t)t];
  return total;
}

void check_at_the_limit() {
  std::mt19937 rng(12345);
  for (int n : {2, 8, 9, 64, 177, 1024, 5000}) {
    const int log2n = ceil_log2((unsigned long long)n);
    for (int emin : {-126, -60, -20, 0, 40}) {
      const int emax = emin + 53 - 1 - log2n - 23;  // the limit exactly
      CHECK(order_free(emax, emin, log2n) && !order_free(emax + 1, emin, log2n), "limit n %d emin %d", n, emin);
      if (emax > 127) continue;
      for (int kind = 0; kind < 3; ++kind) {
        std::vector<float> v((size_t)n);
        for (int k = 0; k < n; ++k) {
          const bool neg = kind == 0 ? false : (rng() & 1u);
          if (kind == 0 || (kind == 1 && k < n / 2)) {
            v[(size_t)k] = make(emax, 0xffffffu, neg);  // the largest magnitude the window admits
          } else {
            const int e = emin + (int)(rng() % (unsigned)(emax - emin + 1));
            uint32_t m = (rng() & 0x7fffffu) | (1u << 23);
            if (e == -126 && (rng() & 1u)) m = 1u + (rng() % 0x7ffffeu);  // denormals among them
            v[(size_t)k] = make(e, m, neg);
          }
        }
        if (kind != 0) v[0] = make(emin, emin == -126 ? 1u : (1u << 23) | 1u, false);  // and the smallest unit
        const __int128 units = exact_units(v, emin);
        const __int128 lim = (__int128)1 << 53;
        CHECK(units < lim && units > -lim, "n %d emin %d kind %d: the exact sum needs more than 53 bits", n, emin, kind);
        const double want = ldexp((double)(long long)units, emin - 23);
        std::vector<int> order((size_t)n);
        for (int k = 0; k < n; ++k) order[(size_t)k] = k;
        const double fwd = sum_in(v, order);
        std::reverse(order.begin(), order.end());
        const double rev = sum_in(v, order);
        std::shuffle(order.begin(), order.end(), rng);
        const double rnd = sum_in(v, order);
        CHECK(dbits(fwd) == dbits(want), "forward n %d emin %d kind %d: %a vs %a", n, emin, kind, fwd, want);
        CHECK(dbits(rev) == dbits(want), "reverse n %d emin %d kind %d: %a vs %a", n, emin, kind, rev, want);
        CHECK(dbits(rnd) == dbits(want), "random n %d emin %d kind %d: %a vs %a", n, emin, kind, rnd, want);
        for (int cols : {1, 3, 16}) {
          const double pre = sum_prefix(v, cols, rng);
          // (a zero sum is +0.0 on every route: x + (-x) and x - x)
          CHECK(dbits(pre) == dbits(want), "prefix n %d emin %d kind %d cols %d: %a vs %a", n, emin, kind, cols, pre, want);
        }
      }
    }
  }
}

// n = 8, exponents 0 .. 27: one bit beyond the limit.  a = (2^24 - 1) 2^4 five times reaches 2^30, where a double's unit is
// 2^-22; b = 1 + 2^-23 then rounds on the way in.  Forward the first b is rounded alone and the sum ends on an odd multiple
// of 2^-22; backwards the three b are exact together, one rounding at the end gives an even one.
void check_beyond_the_limit() {
  const float a = make(27, 0xffffffu, false), b = make(0, (1u << 23) | 1u, false);
  const std::vector<float> v = {a, a, a, a, a, b, b, b};
  CHECK(!order_free(27, 0, ceil_log2(8)) && order_free(26, 0, ceil_log2(8)), "27 - 0 at n = 8 is one beyond");
  std::vector<int> order = {0, 1, 2, 3, 4, 5, 6, 7};
  const double fwd = sum_in(v, order);
  std::reverse(order.begin(), order.end());
  const double rev = sum_in(v, order);
  CHECK(dbits(fwd) != dbits(rev), "the two orders agree: %a %a", fwd, rev);
  const __int128 lim = (__int128)1 << 53;
  CHECK(exact_units(v, 0) >= lim, "the exact sum fits 53 bits");
}

Shape shape_of(double radius, double res, int rows, int cols) {
  te::DiscTable t;
  te::build_disc_table(bounded_radius(radius, res, rows, cols), res, &t);
  Shape s;
  s.R = t.R;
  s.hw0 = t.R >= 0 ? t.hw[0] : 0;
  s.reach = t.reach;
  s.n_ties = t.n_ties();
  s.npoints = t.npoints;
  return s;
}

void check_routes() {
  // the LDS limit on a map taller than every segment: the sliding kernels exactly while their bytes fit
  for (int op : {(int)kMean, (int)kMin}) {
    int last_slide = -1, first_gather = -1;
    for (int h = 0; h <= 6000; ++h) {
      Shape s = {h, h, h, 0, 3ll * h * h + 1};
      const Plan p = plan(op, 1 << 20, 4096, s, 0);
      const size_t bytes = op == kMean ? mean_lds_bytes(1 << 20, h) : min_lds_bytes(1 << 20, h);
      CHECK((p.route == kRouteSlide) == (bytes <= kMaxLds), "op %d hw0 %d: route %d bytes %zu", op, h, p.route, bytes);
      CHECK(p.route == kRouteGather || (p.lds_bytes == bytes && p.seg == 64 + 2 * h), "op %d hw0 %d", op, h);
      CHECK(plan(op, 1 << 20, 4096, s, 2).route == kRouteGather, "option 2 is the gather");
      CHECK(plan(op, 1 << 20, 4096, s, 1).route == p.route, "option 1 is the plan's route while kSlideMinCells is 0");
      if (p.route == kRouteSlide) last_slide = h;
      if (p.route == kRouteGather && first_gather < 0) first_gather = h;
      // a short map: the segment is the map's height whatever the radius
      const Plan q = plan(op, 100, 80, s, 0);
      CHECK(q.route == kRouteSlide && q.seg == (h >= 18 ? 100 : 64 + 2 * h), "op %d hw0 %d on 100 rows: seg %d", op, h, q.seg);
    }
    CHECK(first_gather == last_slide + 1 && last_slide > 300, "op %d: one threshold (%d, %d)", op, last_slide, first_gather);
    if (op == kMean) CHECK(last_slide == 2441, "Mean: (64 + 2 h + 1 + 512) * 12 + 8 <= 65536 up to h = 2441, got %d", last_slide);
  }
  // the Min tables: a run is read at level floor(log2(width)) < levels, width <= min(2 hw0 + 1, seg)
  for (int rows : {1, 5, 64, 100, 4096})
    for (int h = 0; h < 200; ++h) {
      const long long seg = segment_len(rows, h), w = std::min<long long>(2ll * h + 1, seg);
      CHECK((1ll << (min_levels(rows, h) - 1)) <= w && w < (1ll << min_levels(rows, h)), "levels rows %d hw0 %d", rows, h);
    }
  // more column groups than a grid holds: the gather, in strides
  {
    Shape s = {1, 1, 1, 0, 5};
    const Plan p = plan(kMean, 64, 16 * 65535 + 1, s, 1);
    CHECK(p.route == kRouteGather && p.grid_y == kMaxGridY, "grid limit: route %d grid_y %u", p.route, p.grid_y);
    CHECK(plan(kMean, 64, 16 * 65535, s, 1).route == kRouteSlide, "grid limit, below");
  }
  // the bounded radius: the same cells of the map, no tie among them, a table of O(rows + cols)
  for (double cells : {1e3, 1e9, 1e300}) {
    const Shape s = shape_of(cells * 0.05, 0.05, 70, 37);
    CHECK(s.R >= 70 + 37 && s.R <= 70 + 37 + 3, "bounded radius: R %d", s.R);
    te::DiscTable t;
    te::build_disc_table(bounded_radius(cells * 0.05, 0.05, 70, 37), 0.05, &t);
    for (int k = 0; k < t.n_ties(); ++k)
      CHECK(abs(t.ties[2 * (size_t)k]) >= 70 || abs(t.ties[2 * (size_t)k + 1]) >= 37, "a tie of the bounded disc inside the map");
    for (int b = 0; b < 37; ++b) CHECK(t.hw[(size_t)b] >= 69, "bounded disc: column offset %d reaches %d rows", b, t.hw[(size_t)b]);
  }
  CHECK(bounded_radius(0.175, 0.05, 70, 37) == 0.175, "a radius inside the map is kept");
  // the disc is symmetric (the gather reads hw by row offset), radius 0 is the centre as a tie
  for (double cells : {0.0, 0.5, 1.5, 3.0, 3.5, 5.0, 7.5, 40.0}) {
    te::DiscTable t;
    te::build_disc_table(cells * 0.05, 0.05, &t);
    CHECK(t.R < 0 || t.hw[0] == t.R, "hw[0] %d R %d at %g cells", t.R < 0 ? 0 : t.hw[0], t.R, cells);
    for (int b = 0; b <= t.R; ++b)
      for (int a = 0; a <= t.R; ++a) CHECK((a <= t.hw[(size_t)b]) == (b <= t.hw[(size_t)a]), "symmetry at %g cells (%d, %d)", cells, a, b);
    if (cells == 0.0) CHECK(t.R == -1 && t.n_ties() == 1 && t.ties[0] == 0 && t.ties[1] == 0, "radius 0");
  }
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 8 && !strcmp(argv[1], "route")) {
    const int op = atoi(argv[2]), rows = atoi(argv[3]), cols = atoi(argv[4]), opt = atoi(argv[7]);
    const Shape s = shape_of(atof(argv[5]), atof(argv[6]), rows, cols);
    const Plan p = plan(op, rows, cols, s, opt);
    printf("%s %zu %d %d %d %d %d %d %d %lld\n", p.route == kRouteSlide ? "slide" : "gather", p.lds_bytes, p.seg, p.levels, p.log2n, s.R, s.hw0, s.reach,
           s.n_ties, s.npoints);
    return 0;
  }
  if (argc == 5 && !strcmp(argv[1], "free")) {
    printf("%d\n", order_free(atoi(argv[2]), atoi(argv[3]), atoi(argv[4])) ? 1 : 0);
    return 0;
  }
  check_at_the_limit();
  check_beyond_the_limit();
  check_routes();
  printf("%d checks, %d failed checks\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
