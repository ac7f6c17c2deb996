// CPU check of the region plans (traversability_estimation_amd/csrc/te_region_plan.h): te_run_median_fill_region and
// te_run_radius_filter_region.  tests/test_region_plan.py runs it plain and under the sanitizers.
//   region_plan_check                                              the checks below
//   region_plan_check median ROWS COLS R_FILL R_EXIST K OPT ROW0 COL0 H W   prints "tile|any reach out_row0 out_col0 out_h out_w blocks"
//   region_plan_check radius OP ROWS COLS RADIUS RES OPT ROW0 COL0 H W      prints "slide|gather reach out_row0 out_col0 out_h out_w grid_x grid_y"
// Checks, for every rectangle of small maps (and a few rectangles of maps of several tiles), k in 0..2, r in 0..3, both routes:
//   - the launch geometry of every route gives every cell of `out` exactly one owner, and no owner outside `out`;
//   - every rectangle a stage computes or reads lies in the map, and a stage reads only what the stage before computed;
//   - the mask stages run on their rectangles over scratch full of garbage give, on `out`, the bytes of the whole-map mask of the
//     updated input, and the whole-map masks of the earlier and the updated input agree outside `out`.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "te_disc_table.h"
#include "te_region_plan.h"

using namespace te;
using te::region::Rect;

namespace {
int g_failed = 0;
long long g_checks = 0;
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

bool in_map(const Rect& r, int rows, int cols) { return r.i0 >= 0 && r.j0 >= 0 && r.i0 < r.i1 && r.j0 < r.j1 && r.i1 <= rows && r.j1 <= cols; }

struct Owners {
  int rows, cols;
  std::vector<int> n;
  bool outside = false;
  Owners(int r, int c) : rows(r), cols(c), n((size_t)r * c, 0) {}
  void own(int i, int j) {
    if (i < 0 || i >= rows || j < 0 || j >= cols)
      outside = true;
    else
      ++n[(size_t)j * rows + i];
  }
  // every cell of `out` once, every other cell never
  bool exactly(const Rect& out) const {
    if (outside) return false;
    for (int j = 0; j < cols; ++j)
      for (int i = 0; i < rows; ++i) {
        const bool in = i >= out.i0 && i < out.i1 && j >= out.j0 && j < out.j1;
        if (n[(size_t)j * rows + i] != (in ? 1 : 0)) return false;
      }
    return true;
  }
};

// ---- the mask passes as the kernels compute a cell (te_median.hip: morph_cell, or_cell) ----
uint8_t morph_cell(const std::vector<uint8_t>& s, int rows, int cols, int i, int j, bool erode) {
  int all = 1, any = 0;
  for (int jj = j > 0 ? j - 1 : 0; jj <= (j < cols - 1 ? j + 1 : cols - 1); ++jj)
    for (int ii = i > 0 ? i - 1 : 0; ii <= (i < rows - 1 ? i + 1 : rows - 1); ++ii) {
      const int b = s[(size_t)jj * rows + ii] != 0;
      all &= b;
      any |= b;
    }
  return (uint8_t)(erode ? all : any);
}
uint8_t or_cell(const std::vector<uint8_t>& s, int rows, int cols, int i, int j, int r, bool along_rows) {
  int any = 0;
  if (along_rows) {
    for (int ii = i > r ? i - r : 0; ii <= ((rows - 1 - i > r) ? i + r : rows - 1); ++ii) any |= s[(size_t)j * rows + ii] != 0;
  } else {
    for (int jj = j > r ? j - r : 0; jj <= ((cols - 1 - j > r) ? j + r : cols - 1); ++jj) any |= s[(size_t)jj * rows + i] != 0;
  }
  return (uint8_t)any;
}
template <class F>
void over(const Rect& q, F f) {
  for (size_t k = 0; k < region::cells(q); ++k) {
    int i, j;
    region::cell_of(q, k, &i, &j);
    f(i, j);
  }
}
std::vector<uint8_t> whole_mask(const std::vector<uint8_t>& v, int rows, int cols, int r_fill, int k) {
  const Rect all = {0, 0, rows, cols};
  std::vector<uint8_t> a = v, b(v.size());
  for (int s = 0; s < 2 * k; ++s) {
    over(all, [&](int i, int j) { b[(size_t)j * rows + i] = morph_cell(a, rows, cols, i, j, s < k); });
    a.swap(b);
  }
  over(all, [&](int i, int j) { b[(size_t)j * rows + i] = or_cell(a, rows, cols, i, j, r_fill, true); });
  over(all, [&](int i, int j) { a[(size_t)j * rows + i] = or_cell(b, rows, cols, i, j, r_fill, false); });
  return a;
}
// the launches of median::launch_region, on scratch that holds garbage wherever no stage wrote
std::vector<uint8_t> region_mask(const std::vector<uint8_t>& v, const median::RegionPlan& p, std::vector<uint8_t> stored, std::mt19937& rng) {
  const int rows = p.rows, cols = p.cols;
  std::vector<uint8_t> tmp[2] = {std::vector<uint8_t>(v.size()), std::vector<uint8_t>(v.size())};
  for (auto& t : tmp)
    for (auto& x : t) x = (uint8_t)(rng() & 3u);
  over(median::mask_stage_rect(p, 0), [&](int i, int j) { tmp[0][(size_t)j * rows + i] = v[(size_t)j * rows + i]; });
  int cur = 0;
  for (int s = 0; s < 2 * p.iterations; ++s) {
    over(median::mask_stage_rect(p, s + 1), [&](int i, int j) { tmp[cur ^ 1][(size_t)j * rows + i] = morph_cell(tmp[cur], rows, cols, i, j, s < p.iterations); });
    cur ^= 1;
  }
  over(median::row_or_rect(p), [&](int i, int j) { tmp[cur ^ 1][(size_t)j * rows + i] = or_cell(tmp[cur], rows, cols, i, j, p.r_fill, true); });
  over(p.out, [&](int i, int j) { stored[(size_t)j * rows + i] = or_cell(tmp[cur ^ 1], rows, cols, i, j, p.r_fill, false); });
  return stored;
}

void check_median(int rows, int cols, const Rect& dirty, int r_fill, int r_exist, int k, int option, std::mt19937& rng, bool simulate) {
  const median::RegionPlan p = median::region_plan(rows, cols, r_fill, r_exist, k, option, dirty);
  const long long reach = std::max<long long>(r_fill + 2 * k, r_exist);
  const Rect want = region::grown(dirty, reach, reach, rows, cols);
  CHECK(p.reach == reach && p.out.i0 == want.i0 && p.out.j0 == want.j0 && p.out.i1 == want.i1 && p.out.j1 == want.j1, "out %dx%d r %d %d k %d", rows, cols, r_fill,
        r_exist, k);
  CHECK(in_map(p.out, rows, cols) && region::inside(dirty, p.out), "out in map %dx%d", rows, cols);
  CHECK(p.k.route == (option == 2 || !median::tile_fits(p.k.r) ? median::kRouteAny : median::kRouteTile), "route");
  // the stages
  Rect before = median::mask_stage_rect(p, 0);
  CHECK(in_map(before, rows, cols), "V in map");
  for (int s = 1; s <= 2 * k; ++s) {
    const Rect q = median::mask_stage_rect(p, s);
    CHECK(in_map(q, rows, cols) && region::inside(median::mask_stage_reads(p, s), before), "stage %d reads the stage before", s);
    before = q;
  }
  CHECK(in_map(median::row_or_rect(p), rows, cols) && region::inside(median::row_or_reads(p), before), "row OR reads the last morph");
  CHECK(region::inside(median::col_or_reads(p), median::row_or_rect(p)), "column OR reads the row OR");
  CHECK(in_map(median::median_reads(p), rows, cols), "median reads in map");
  // the owners
  Owners o(rows, cols);
  if (p.k.route == median::kRouteTile) {
    CHECK(p.k.blocks == (size_t)p.k.tiles_x * p.k.tiles_y && p.k.lds_bytes + median::kTileStaticLds <= median::kLdsBudget, "tile launch");
    for (size_t b = 0; b < p.k.blocks; ++b) {
      const int tx = (int)(b % (size_t)p.k.tiles_x), ty = (int)((b / (size_t)p.k.tiles_x) % (size_t)p.k.tiles_y);
      for (int lj = 0; lj < median::kTileCols; ++lj)
        for (int li = 0; li < median::kTileRows; ++li) {
          int i, j;
          if (median::tile_owner(p, tx, ty, li, lj, &i, &j)) o.own(i, j);
        }
    }
  } else {
    CHECK(p.any_blocks == (region::cells(p.out) + 255) / 256, "any blocks");
    for (size_t idx = 0; idx < p.any_blocks * 256; ++idx)
      if (idx < region::cells(p.out)) {
        int i, j;
        region::cell_of(p.out, idx, &i, &j);
        o.own(i, j);
      }
  }
  CHECK(o.exactly(p.out), "owners %dx%d dirty (%d,%d)-(%d,%d) r %d %d k %d route %d", rows, cols, dirty.i0, dirty.j0, dirty.i1, dirty.j1, r_fill, r_exist, k, p.k.route);
  if (!simulate) return;
  // the mask: earlier input, then other values inside `dirty`
  std::vector<uint8_t> v0((size_t)rows * cols), v1;
  for (auto& x : v0) x = (rng() % 4u) != 0;
  v1 = v0;
  over(dirty, [&](int i, int j) { v1[(size_t)j * rows + i] = (uint8_t)(rng() & 1u); });
  const std::vector<uint8_t> m0 = whole_mask(v0, rows, cols, r_fill, k), m1 = whole_mask(v1, rows, cols, r_fill, k);
  const std::vector<uint8_t> got = region_mask(v1, p, m0, rng);
  CHECK(got == m1, "region mask %dx%d dirty (%d,%d)-(%d,%d) r %d k %d", rows, cols, dirty.i0, dirty.j0, dirty.i1, dirty.j1, r_fill, k);
}

radius::Shape shape_of(double rad, double res, int rows, int cols) {
  DiscTable t;
  build_disc_table(radius::bounded_radius(rad, res, rows, cols), res, &t);
  radius::Shape s;
  s.R = t.R;
  s.hw0 = t.R >= 0 ? t.hw[0] : 0;
  s.reach = t.reach;
  s.n_ties = t.n_ties();
  s.npoints = t.npoints;
  return s;
}

void check_radius(int op, int rows, int cols, const Rect& dirty, const radius::Shape& s, int option) {
  const radius::RegionPlan p = radius::region_plan(op, rows, cols, s, option, dirty);
  const radius::Plan whole = radius::plan(op, rows, cols, s, option);
  const Rect want = region::grown(dirty, s.reach, s.reach, rows, cols);
  CHECK(p.reach == s.reach && p.out.i0 == want.i0 && p.out.j0 == want.j0 && p.out.i1 == want.i1 && p.out.j1 == want.j1, "radius out");
  CHECK(in_map(p.out, rows, cols), "radius out in map");
  CHECK(p.k.route == whole.route && p.k.lds_bytes == whole.lds_bytes && p.k.seg == whole.seg && p.k.levels == whole.levels && p.k.log2n == whole.log2n, "the whole call's route");
  CHECK(p.k.grid_x >= 1 && p.k.grid_y >= 1 && p.k.grid_y <= radius::kMaxGridY && p.k.grid_x <= whole.grid_x && p.k.grid_y <= whole.grid_y, "grid");
  Owners o(rows, cols);
  for (unsigned by = 0; by < p.k.grid_y; ++by)
    for (unsigned bx = 0; bx < p.k.grid_x; ++bx)
      for (int ty = 0; ty < radius::kWaves; ++ty)
        for (int tx = 0; tx < radius::kTX; ++tx) {
          const int i = p.out.i0 + (int)bx * radius::kTX + tx;
          if (p.k.route == radius::kRouteSlide) {
            const int i0 = p.out.i0 + (int)bx * radius::kTX, j0 = p.out.j0 + (int)by * radius::kTY;
            if (tx == 0 && ty == 0) CHECK(i0 < rows && j0 < cols, "tile origin in map");  // the staged segment is not empty
            for (int c = 0; c < radius::kTY / radius::kWaves; ++c) {
              const int j = j0 + ty + c * radius::kWaves;
              if (i < p.out.i1 && j < p.out.j1) o.own(i, j);
            }
          } else {
            if (i >= p.out.i1) continue;
            for (long long j = (long long)p.out.j0 + (long long)by * radius::kWaves + ty; j < p.out.j1; j += (long long)p.k.grid_y * radius::kWaves) o.own(i, (int)j);
          }
        }
  CHECK(o.exactly(p.out), "radius owners %dx%d dirty (%d,%d)-(%d,%d) reach %d route %d", rows, cols, dirty.i0, dirty.j0, dirty.i1, dirty.j1, s.reach, p.k.route);
}

template <class F>
void every_rect(int rows, int cols, F f) {
  for (int i0 = 0; i0 < rows; ++i0)
    for (int i1 = i0 + 1; i1 <= rows; ++i1)
      for (int j0 = 0; j0 < cols; ++j0)
        for (int j1 = j0 + 1; j1 <= cols; ++j1) f(Rect{i0, j0, i1, j1});
}

void checks() {
  std::mt19937 rng(20240);
  const int small_rows[] = {1, 2, 3, 7, 12}, small_cols[] = {1, 2, 5, 9};
  const double res = 0.05, radii[] = {0.0, 1.5 * res, 2.0 * res, 3.0 * res};
  for (int rows : small_rows)
    for (int cols : small_cols) {
      radius::Shape shapes[4];
      for (int q = 0; q < 4; ++q) shapes[q] = shape_of(radii[q], res, rows, cols);
      long long n = 0;
      every_rect(rows, cols, [&](const Rect& d) {
        for (int k = 0; k <= 2; ++k)
          for (int r = 0; r <= 3; ++r)
            for (int r_exist : {-1, 1, 3})
              for (int option : {0, 2}) check_median(rows, cols, d, r, r_exist, k, option, rng, r_exist == -1 && option == 0 && (n++ % 3) == 0);
        for (int q = 0; q < 4; ++q)
          for (int op : {radius::kMean, radius::kMin})
            for (int option : {0, 2}) check_radius(op, rows, cols, d, shapes[q], option);
      });
    }
  // maps of several tiles: rectangles at the corners, across tile borders, a strip, the whole map
  const int big[][2] = {{67, 45}, {131, 70}, {200, 33}};
  for (const auto& m : big) {
    const int rows = m[0], cols = m[1];
    const Rect rects[] = {{0, 0, 8, 8},           {rows - 8, cols - 8, rows, cols}, {0, cols - 8, 8, cols}, {rows - 8, 0, rows, 8}, {rows / 2, cols / 2, rows / 2 + 1, cols / 2 + 1},
                          {0, 20, rows, 25},      {0, 0, rows, cols},               {60, 10, 67, 20},       {1, 1, 66, 18}};
    for (const Rect& d : rects) {
      for (int k : {0, 2, 4})
        for (int r : {0, 1, 2, 16})
          for (int r_exist : {-1, 1})
            for (int option : {0, 1, 2}) check_median(rows, cols, d, r, r_exist, k, option, rng, option == 0 && r_exist == -1 && r <= 2);
      for (double cells : {0.0, 1.5, 2.0, 3.0, 9.0, 40.0}) {
        const radius::Shape s = shape_of(cells * res, res, rows, cols);
        for (int op : {radius::kMean, radius::kMin})
          for (int option : {0, 1, 2}) check_radius(op, rows, cols, d, s, option);
      }
    }
  }
  // the rectangle checks of te_run_chain_region
  CHECK(region::valid_rect(5, 7, 0, 0, 5, 7) && region::valid_rect(5, 7, 4, 6, 1, 1), "valid");
  CHECK(!region::valid_rect(5, 7, -1, 0, 2, 2) && !region::valid_rect(5, 7, 0, 0, 6, 7) && !region::valid_rect(5, 7, 0, 0, 0, 1) && !region::valid_rect(5, 7, 4, 0, 2, 1) &&
            !region::valid_rect(5, 7, 0, 0x7fffffff, 1, 1) && !region::valid_rect(5, 7, 1, 1, 0x7fffffff, 0x7fffffff),
        "invalid");
  // a growth beyond int
  const Rect g = region::grown(Rect{3, 4, 5, 6}, 0x7fffffffll * 3, 1, 10, 12);
  CHECK(g.i0 == 0 && g.i1 == 10 && g.j0 == 3 && g.j1 == 7, "grown");
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 12 && !strcmp(argv[1], "median")) {
    int a[10];
    for (int k = 0; k < 10; ++k) a[k] = atoi(argv[2 + k]);
    if (!region::valid_rect(a[0], a[1], a[6], a[7], a[8], a[9])) return 2;
    const median::RegionPlan p = median::region_plan(a[0], a[1], a[2], a[3], a[4], a[5], Rect{a[6], a[7], a[6] + a[8], a[7] + a[9]});
    printf("%s %lld %d %d %d %d %zu\n", p.k.route == median::kRouteTile ? "tile" : "any", p.reach, p.out.i0, p.out.j0, region::height(p.out), region::width(p.out),
           p.k.route == median::kRouteTile ? p.k.blocks : p.any_blocks);
    return 0;
  }
  if (argc == 12 && !strcmp(argv[1], "radius")) {
    const int op = atoi(argv[2]), rows = atoi(argv[3]), cols = atoi(argv[4]), opt = atoi(argv[7]);
    const double rad = atof(argv[5]), res = atof(argv[6]);
    const int r0 = atoi(argv[8]), c0 = atoi(argv[9]), h = atoi(argv[10]), w = atoi(argv[11]);
    if (!region::valid_rect(rows, cols, r0, c0, h, w)) return 2;
    const radius::RegionPlan p = radius::region_plan(op, rows, cols, shape_of(rad, res, rows, cols), opt, Rect{r0, c0, r0 + h, c0 + w});
    printf("%s %d %d %d %d %d %u %u\n", p.k.route == radius::kRouteSlide ? "slide" : "gather", p.reach, p.out.i0, p.out.j0, region::height(p.out), region::width(p.out),
           p.k.grid_x, p.k.grid_y);
    return 0;
  }
  checks();
  printf("region_plan_check: %lld checks, %d failed checks\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
