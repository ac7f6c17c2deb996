// distance_plan_check.cpp -- csrc/te_distance_plan.h and the per-cell routines of csrc/te_distance.h on the CPU
// (tests/test_distance_plan.py; plain and under the sanitizers):
//   the cap       cap2 and R against the defining loop over k, the ties and the refusals;
//   rectangles    single-seed flips: a cell outside `out` cannot change, every seed that reaches a cell of `out` lies in `in`,
//                 and each pass reads only what the rectangle before it holds;
//   geometry      every cell of g has exactly one owner in pass 1, every cell of out exactly one in pass 2, and a tile of the
//                 tiled route stages no more columns than its LDS holds;
//   routines      column_nearest and row_min, driven over the plan's geometry exactly as the kernels drive them, against brute
//                 force on every cell, with the steps of row_min counted.
//   distance_plan_check route ROWS COLS MAX_DISTANCE RES OPTION [ROW0 COL0 H W]  prints the plan of a call: route, cap2, R, LDS bytes, the blocks
//   of both passes, seg_chunks, the rectangle out, p1_segs, the rectangles g and in (each rectangle as row0 col0 h w).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "te_distance_plan.h"

using namespace te;
using namespace te::distance;

namespace {
int g_failed = 0, g_checks = 0;
#define CHECK(cond, ...)              \
  do {                                \
    ++g_checks;                       \
    if (!(cond)) {                    \
      if (++g_failed <= 20) {         \
        printf("FAILED %s: ", #cond); \
        printf(__VA_ARGS__);          \
        printf("\n");                 \
      }                               \
    }                                 \
  } while (0)

uint32_t isqrt(uint32_t v) {
  uint32_t r = 0;
  while ((uint64_t)(r + 1) * (r + 1) <= v) ++r;
  return r;
}

void check_cap() {
  const double ress[] = {0.005, 0.01, 0.03, 0.05, 0.1, 0.25, 1.0, 2.0};
  const double cells[] = {0.01, 0.5, 1.0, 1.4142135623730951, 1.5, 2.0, 2.23606797749979, 3.0, 5.0, 7.5, 10.0, 40.0, 200.0};
  for (double res : ress)
    for (double n : cells) {
      const double md = n * res, q = md * md, r2 = res * res;
      uint32_t k = 0;
      while ((double)(k + 1) * r2 <= q) ++k;
      uint32_t cap2 = 0;
      int R = -1;
      CHECK(cap_of(md, res, &cap2, &R), "res %g md %g", res, md);
      CHECK(cap2 == k && (uint32_t)R == isqrt(k), "res %g md %g: cap2 %u R %d, loop %u", res, md, cap2, R, k);
    }
  const double ties[][2] = {{0.5, 0.05}, {0.15, 0.03}};
  for (const auto& t : ties) {
    uint32_t k = 0, cap2 = 0;
    int R = -1;
    while ((double)(k + 1) * (t[1] * t[1]) <= t[0] * t[0]) ++k;
    CHECK(cap_of(t[0], t[1], &cap2, &R) && cap2 == k && (uint32_t)R == isqrt(k), "tie %g at %g: cap2 %u, loop %u", t[0], t[1], cap2, k);
  }
  uint32_t cap2 = 7;
  int R = 7;
  CHECK(!cap_of(0.0, 0.05, &cap2, &R) && !cap_of(-1.0, 0.05, &cap2, &R) && !cap_of(NAN, 0.05, &cap2, &R) && !cap_of(INFINITY, 0.05, &cap2, &R), "refusals");
  CHECK(!cap_of(1e200, 0.05, &cap2, &R), "max_distance squared overflows");
  CHECK(!cap_of(32768.0 * 0.05, 0.05, &cap2, &R) && !cap_of(32768.0, 1.0, &cap2, &R), "R = 32768 is refused");
  CHECK(cap_of(32767.5, 1.0, &cap2, &R) && R == kMaxReach && (double)cap2 <= 32767.5 * 32767.5 && (double)(cap2 + 1) > 32767.5 * 32767.5, "R = 32767: %d %u", R, cap2);
  CHECK(cap_of(1e-300, 0.05, &cap2, &R) && cap2 == 0 && R == 0, "a tiny cap is R = 0");
}

bool in_rect(const region::Rect& r, int i, int j) { return i >= r.i0 && i < r.i1 && j >= r.j0 && j < r.j1; }

void check_rects_of(int rows, int cols, int R, const region::Rect& dirty) {
  const uint32_t cap2 = (uint32_t)(R + 1) * (uint32_t)(R + 1) - 1;  // the largest cap of this reach
  const Plan p = plan(rows, cols, cap2, R, 0, dirty);
  const region::Rect whole = {0, 0, rows, cols};
  bool ok = region::inside(dirty, p.out) && region::inside(p.out, p.g) && region::inside(p.g, p.in) && region::inside(p.in, whole);
  ok = ok && p.g.i0 == p.out.i0 && p.g.i1 == p.out.i1 && p.in.j0 == p.g.j0 && p.in.j1 == p.g.j1;
  // a single seed at (si, sj), flipped on an empty map, changes exactly the cells within cap2 of it
  for (int si = 0; si < rows && ok; ++si)
    for (int sj = 0; sj < cols && ok; ++sj)
      for (int i = 0; i < rows && ok; ++i)
        for (int j = 0; j < cols; ++j) {
          const uint32_t d2 = (uint32_t)((i - si) * (i - si) + (j - sj) * (j - sj));
          if (d2 > cap2) continue;
          if (in_rect(dirty, si, sj) && !in_rect(p.out, i, j)) ok = false;  // a cell outside out changed
          if (in_rect(p.out, i, j) && !in_rect(p.in, si, sj)) ok = false;    // a seed that reaches out is not read
        }
  // pass 2 reads g within R columns of out, pass 1 the input within R rows of g
  for (int i = p.out.i0; i < p.out.i1 && ok; ++i)
    for (int j = p.out.j0; j < p.out.j1; ++j)
      for (int d = -R; d <= R; ++d) {
        if (j + d >= 0 && j + d < cols && !in_rect(p.g, i, j + d)) ok = false;
      }
  for (int i = p.g.i0; i < p.g.i1 && ok; ++i)
    for (int j = p.g.j0; j < p.g.j1; ++j)
      for (int d = -R; d <= R; ++d) {
        if (i + d >= 0 && i + d < rows && !in_rect(p.in, i + d, j)) ok = false;
      }
  // nothing is read farther than 2 R from the rectangle
  ok = ok && p.in.i0 >= dirty.i0 - 2 * R && p.in.j0 >= dirty.j0 - 2 * R && p.in.i1 <= dirty.i1 + 2 * R && p.in.j1 <= dirty.j1 + 2 * R;
  CHECK(ok, "%d x %d R %d dirty [%d,%d)x[%d,%d)", rows, cols, R, dirty.i0, dirty.i1, dirty.j0, dirty.j1);
}

void check_rects() {
  const int maps[][2] = {{1, 1}, {1, 9}, {12, 1}, {2, 3}, {5, 4}, {7, 9}, {12, 9}};
  for (const auto& m : maps) {
    const int rows = m[0], cols = m[1], step = rows * cols > 63 ? 3 : 1;  // (the largest map: every third origin and size)
    for (int R = 0; R <= 4; ++R)
      for (int i0 = 0; i0 < rows; i0 += step)
        for (int j0 = 0; j0 < cols; j0 += step)
          for (int h = 1; i0 + h <= rows; h += step)
            for (int w = 1; j0 + w <= cols; w += step) check_rects_of(rows, cols, R, region::Rect{i0, j0, i0 + h, j0 + w});
    for (int R = 0; R <= 4; ++R) check_rects_of(rows, cols, R, region::Rect{0, 0, rows, cols});
  }
}

// the owners of the cells of g and out under the plan's launch geometry
void check_owners(const Plan& p, const char* what) {
  const int gh = region::height(p.g), gw = region::width(p.g), oh = region::height(p.out), ow = region::width(p.out);
  std::vector<int> own_g((size_t)gh * gw, 0), own_o((size_t)oh * ow, 0);
  bool ok = p.fits && p.seg_chunks >= 1 && p.seg_chunks <= kMaxSegChunks;
  for (unsigned long long b = 0; b < p.p1_blocks; ++b)
    for (int wave = 0; wave < kWaves; ++wave) {
      int i0, i1, j;
      if (!p1_unit(p, b, wave, &i0, &i1, &j)) continue;
      if (i1 - i0 > p.seg_chunks * kLanes || i0 < p.g.i0 || i1 > p.g.i1 || j < p.g.j0 || j >= p.g.j1) ok = false;
      for (int i = i0; i < i1 && ok; ++i) ++own_g[(size_t)(j - p.g.j0) * gh + (i - p.g.i0)];
    }
  for (int v : own_g) ok = ok && v == 1;
  CHECK(ok, "%s: pass 1 owners", what);
  ok = true;
  for (unsigned long long b = 0; b < p.p2_blocks; ++b) {
    int i0, j0, c0, c1;
    p2_tile(p, b, &i0, &j0);
    p2_columns(p, j0, &c0, &c1);
    if (c0 < p.g.j0 || c1 > p.g.j1 || c0 >= c1) ok = false;
    if (p.route == kRouteTiled && ((c1 - c0) > p.lds_cols || (size_t)(c1 - c0) * kTI * sizeof(uint16_t) > p.lds_bytes || p.lds_bytes > kMaxLds)) ok = false;
    for (int wave = 0; wave < kWaves; ++wave)
      for (int lane = 0; lane < kLanes; ++lane)
        for (int k = 0; k < kCellsPerLane; ++k) {
          int i, j;
          if (!p2_cell(p, i0, j0, wave, lane, k, &i, &j)) continue;
          // the columns of g its row reaches are the tile's
          const int a = j - p.R < p.g.j0 ? p.g.j0 : j - p.R, z = j + p.R >= p.g.j1 ? p.g.j1 - 1 : j + p.R;
          if (!in_rect(p.out, i, j) || a < c0 || z >= c1) ok = false;
          if (ok) ++own_o[(size_t)(j - p.out.j0) * oh + (i - p.out.i0)];
        }
  }
  for (int v : own_o) ok = ok && v == 1;
  CHECK(ok, "%s: pass 2 owners", what);
}

void check_geometry() {
  const int shapes[][2] = {{1, 1}, {5, 200}, {70, 37}, {130, 96}, {257, 64}, {4096, 5}, {3, 700}};
  const int Rs[] = {0, 1, 3, 9, 40, 80, 240, 300, 5000};
  char what[128];
  for (const auto& s : shapes)
    for (int R : Rs)
      for (int opt = 0; opt <= 2; ++opt) {
        const int rows = s[0], cols = s[1];
        const uint32_t cap2 = (uint32_t)R * (uint32_t)R;
        snprintf(what, sizeof(what), "%d x %d R %d option %d", rows, cols, R, opt);
        const Plan p = plan(rows, cols, cap2, R, opt, region::Rect{0, 0, rows, cols});
        check_owners(p, what);
        CHECK(p.route == (opt == 2 ? kRouteAny : p.route) && (p.route == kRouteAny || p.lds_bytes <= kMaxLds), "%s: route", what);
        if (opt == 0) CHECK(p.route == kRouteAny || R <= kTiledMaxReach, "%s: by plan", what);
        if (opt == 1) CHECK((p.route == kRouteTiled) == ((size_t)(kTJ + 2ll * R < cols ? kTJ + 2ll * R : cols) * kTI * 2 <= kMaxLds), "%s: wherever it fits", what);
        if (rows > 10 && cols > 10) {
          const Plan q = plan(rows, cols, cap2, R, opt, region::Rect{rows / 2, cols / 3, rows / 2 + 3, cols / 3 + 7});
          snprintf(what, sizeof(what), "%d x %d R %d option %d, a region", rows, cols, R, opt);
          check_owners(q, what);
        }
      }
}

// Pass 1 as k_distance_columns drives column_nearest: the seeds of 64 rows as a mask, the nearest seed before and behind the
// chunk as distances.  seed: [cols][rows] of the map
void pass1(const Plan& p, const std::vector<uint8_t>& seed, std::vector<uint16_t>* g) {
  const int gh = region::height(p.g);
  g->assign(p.g_cells, 0xffff);
  for (unsigned long long b = 0; b < p.p1_blocks; ++b)
    for (int wave = 0; wave < kWaves; ++wave) {
      int i0, i1, j;
      if (!p1_unit(p, b, wave, &i0, &i1, &j)) continue;
      const uint8_t* col = &seed[(size_t)j * p.rows];
      const long long low = (long long)i0 - p.R > p.in.i0 ? (long long)i0 - p.R : p.in.i0, high = p.in.i1;
      for (long long row0 = i0; row0 < i1; row0 += kLanes) {
        uint64_t m = 0;
        for (int l = 0; l < kLanes; ++l)
          if (row0 + l < high && col[row0 + l]) m |= 1ull << l;
        int before = kNone, after = kNone;
        for (long long r = row0 - 1; r >= low; --r)
          if (col[r]) {
            before = (int)(row0 - r);
            break;
          }
        for (long long r = row0 + kLanes; r < high && r < (long long)i1 + p.R + kLanes; ++r)
          if (col[r]) {
            after = (int)(r - (row0 + kLanes - 1));
            break;
          }
        for (int l = 0; l < kLanes && row0 + l < i1; ++l)
          (*g)[(size_t)(j - p.g.j0) * gh + (size_t)(row0 + l - p.g.i0)] = (uint16_t)column_nearest(m, l, before, after, p.R + 1);
      }
    }
}

unsigned g_rng = 12345u;
unsigned rnd() { return g_rng = g_rng * 1664525u + 1013904223u; }

void check_routines_on(int rows, int cols, int R, int density_permille, const region::Rect& dirty, long long* steps_all, long long* steps_full) {
  std::vector<uint8_t> seed((size_t)rows * cols);
  for (auto& s : seed) s = (int)(rnd() >> 8) % 1000 < density_permille;
  const uint32_t cap2 = (uint32_t)R * (uint32_t)R + (R > 0 ? (uint32_t)R : 0u);  // R^2 <= cap2 < (R + 1)^2
  const Plan p = plan(rows, cols, cap2, R, 0, dirty);
  std::vector<uint16_t> g;
  pass1(p, seed, &g);
  const int gh = region::height(p.g);
  bool ok1 = true, ok2 = true, ok3 = true;
  for (int j = p.g.j0; j < p.g.j1; ++j)
    for (int i = p.g.i0; i < p.g.i1; ++i) {
      int want = R + 1;
      for (int r = 0; r < rows; ++r)
        if (seed[(size_t)j * rows + r] && abs(r - i) < want) want = abs(r - i);
      if (g[(size_t)(j - p.g.j0) * gh + (i - p.g.i0)] != want) ok1 = false;
    }
  CHECK(ok1, "column_nearest: %d x %d R %d at %d permille", rows, cols, R, density_permille);
  for (unsigned long long b = 0; b < p.p2_blocks; ++b) {
    int i0, j0, c0, c1;
    p2_tile(p, b, &i0, &j0);
    p2_columns(p, j0, &c0, &c1);
    for (int wave = 0; wave < kWaves; ++wave)
      for (int lane = 0; lane < kLanes; ++lane)
        for (int k = 0; k < kCellsPerLane; ++k) {
          int i, j;
          if (!p2_cell(p, i0, j0, wave, lane, k, &i, &j)) continue;
          const int lo = j - c0 < R ? j - c0 : R, hi = c1 - 1 - j < R ? c1 - 1 - j : R;
          int steps = 0;
          const uint32_t got = row_min(&g[(size_t)(j - p.g.j0) * gh + (i - p.g.i0)], (ptrdiff_t)gh, lo, hi, cap2 + 1, &steps);
          uint32_t want = cap2 + 1;
          for (int c = 0; c < cols; ++c)
            for (int r = 0; r < rows; ++r) {
              const uint32_t d2 = (uint32_t)((r - i) * (r - i) + (c - j) * (c - j));
              if (seed[(size_t)c * rows + r] && d2 < want) want = d2;
            }
          if (got != want) ok2 = false;
          if (steps < 1 || steps > 2 * (int)isqrt(got) + 1 || steps > lo + hi + 1) ok3 = false;
          *steps_all += steps;
          *steps_full += lo + hi + 1;
          // the value: a seed is 0, beyond the cap the cap
          const float v = value_of(got, cap2, 0.05, 123.0f);
          if ((got == 0) != (v == 0.0f) || (got > cap2) != (v == 123.0f)) ok2 = false;
        }
  }
  CHECK(ok2, "row_min: %d x %d R %d at %d permille", rows, cols, R, density_permille);
  CHECK(ok3, "row_min steps: %d x %d R %d at %d permille", rows, cols, R, density_permille);
}

void check_routines() {
  const int shapes[][2] = {{1, 1}, {5, 40}, {70, 37}, {37, 70}, {64, 3}, {65, 9}};
  const int Rs[] = {0, 1, 3, 9, 80}, dens[] = {0, 10, 300, 1000};
  for (const auto& s : shapes)
    for (int R : Rs) {
      for (int d : dens) {
        long long steps = 0, full = 0;
        check_routines_on(s[0], s[1], R, d, region::Rect{0, 0, s[0], s[1]}, &steps, &full);
        if (R >= 3 && d >= 300 && s[1] > 8) CHECK(steps < full, "the early exit is never taken: %d x %d R %d at %d: %lld of %lld", s[0], s[1], R, d, steps, full);
        if (d == 0) CHECK(steps == full, "an empty map walks its whole row: %lld of %lld", steps, full);
      }
      if (s[0] > 20 && s[1] > 20) {  // a region of the same map equals the whole call by construction: the same checks hold on it
        long long steps = 0, full = 0;
        check_routines_on(s[0], s[1], R, 30, region::Rect{s[0] / 2, s[1] / 2, s[0] / 2 + 5, s[1] / 2 + 2}, &steps, &full);
      }
    }
  // the bits of a chunk: every position of the cell and of the seeds on both sides
  bool ok = true;
  for (int l = 0; l < kLanes; ++l)
    for (int s = 0; s < kLanes; ++s) {
      ok = ok && column_nearest(1ull << s, l, kNone, kNone, 100) == abs(l - s);
      ok = ok && column_nearest(0, l, s + 1, kNone, 200) == l + s + 1 && column_nearest(0, l, kNone, s + 1, 200) == 63 - l + s + 1;
      int want = abs(l - s);  // a seed right before and right behind the chunk, saturated at 3
      want = l + 1 < want ? l + 1 : want;
      want = 64 - l < want ? 64 - l : want;
      ok = ok && column_nearest(1ull << s, l, 1, 1, 3) == (want < 3 ? want : 3);
    }
  ok = ok && column_nearest(0, 5, kNone, kNone, 41) == 41 && column_nearest(~0ull, 17, 1, 1, 9) == 0;
  CHECK(ok, "column_nearest on single bits");
}
}  // namespace

int main(int argc, char** argv) {
  if ((argc == 7 || argc == 11) && !strcmp(argv[1], "route")) {
    const int rows = atoi(argv[2]), cols = atoi(argv[3]), opt = atoi(argv[6]);
    uint32_t cap2 = 0;
    int R = 0;
    if (!cap_of(atof(argv[4]), atof(argv[5]), &cap2, &R)) {
      printf("refused\n");
      return 0;
    }
    region::Rect dirty = {0, 0, rows, cols};
    if (argc == 11) dirty = region::Rect{atoi(argv[7]), atoi(argv[8]), atoi(argv[7]) + atoi(argv[9]), atoi(argv[8]) + atoi(argv[10])};
    const Plan p = plan(rows, cols, cap2, R, opt, dirty);
    printf("%s %u %d %zu %llu %llu %d %d %d %d %d", p.route == kRouteTiled ? "tiled" : "any", cap2, R, p.lds_bytes, p.p1_blocks, p.p2_blocks, p.seg_chunks,
           p.out.i0, p.out.j0, region::height(p.out), region::width(p.out));
    printf(" %u %d %d %d %d %d %d %d %d\n", p.p1_segs, p.g.i0, p.g.j0, region::height(p.g), region::width(p.g), p.in.i0, p.in.j0, region::height(p.in),
           region::width(p.in));
    return 0;
  }
  check_cap();
  check_rects();
  check_geometry();
  check_routines();
  printf("%d checks, %d failed checks\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
