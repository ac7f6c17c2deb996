// CPU harness over the plan of te_run_window_expression_region (csrc/te_region_plan.h: wexpr::region_plan, csrc/te_window_plan.h)
// and a lane-by-lane restatement of k_window_expr<region> (csrc/te_window_expr.hip) over the evaluator of te_expr.h
// (tests/test_window_region.py).
//   window_region_check                      the built-in sweep -> "N checks, F failed checks"
//   window_region_check plan ROWS COLS W N_RED N_OUTER OPTION ROW0 COL0 H WD
//                                            -> "separable|direct reach i0 j0 h w tiles staged" (exit 2: rectangle outside the map)
//   window_region_check offlds               -> the smallest odd window the plan does not stage in LDS
//   window_region_check eval TEXT LAYER ROWS COLS W EDGE EMPTY OPTION ROW0 COL0 H WD IN.bin PREV.bin OUT.bin
//                                            OUT = PREV with the cells the region call's lanes own recomputed from IN, tile by
//                                            tile as the kernel does (staged tile, wg_separable, pass A / pass B);
//                                            -> "OK i0 j0 h w separable_workgroups direct_workgroups bad_reads"
// Build: g++ -std=c++17 -O2 -ffp-contract=off.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "te_expr.h"
#include "te_region_plan.h"

using namespace te::expr;
namespace W = te::wexpr;
namespace R = te::region;

namespace {

int g_checks = 0, g_failed = 0;
void check(bool ok, const char* what) {
  ++g_checks;
  if (!ok) {
    ++g_failed;
    printf("FAILED: %s\n", what);
  }
}

struct Stack {
  Vec<1> s[kMaxStack];
  void put(int k, const Vec<1>& v) { s[k] = v; }
  Vec<1> get(int k) const { return s[k]; }
};
struct Res {
  float r[kMaxRed] = {};
  float get(int k) const { return r[k]; }
};
// te_window_expr.hip: At.  A read of a cell of the map that the staged tile does not hold is counted, never made.
struct At {
  const float* in;
  const std::vector<float>* tile;  // nullptr: not staged
  int rows, cols, ia, ja, pitch, tcols;
  float pad;
  long* bad;
  float operator()(int row, int col) const {
    if (row < 0 || row >= rows || col < 0 || col >= cols) return pad;
    if (!tile) return in[(size_t)col * rows + row];
    const int a = row - ia, b = col - ja;
    if (a < 0 || a >= pitch || b < 0 || b >= tcols) {
      ++*bad;
      return pad;
    }
    return (*tile)[(size_t)b * pitch + a];
  }
};

bool finite_f(float v) { return fabsf(v) < INFINITY; }

float direct_cell(const Program& p, int edge, bool empty, int m, At at, int i, int j) {
  Stack st;
  Res res;
  at.pad = NAN;
  const W::Extent e = W::extent(edge, m, at.rows, at.cols, i, j, finite_f(at(i, j)), empty);
  if (!e.visited) return NAN;
  if (edge == W::kMean && e.clipped) at.pad = window_mean_of_finites(at, e.blo, e.bhi, e.bclo, e.bchi);
  for (int level = 0; level < (p.n_outer > 0 ? 2 : 1); ++level)
    for (int r = 0; r < p.n_red; ++r)
      if (p.red_level[r] == level) res.r[r] = window_reduce(p, r, st, res, at, e.rlo, e.rhi, e.clo, e.chi);
  const WindowSource<Res> src{0.0f, &res};
  return run<1>(p, 0, p.n_main, st, src).v[0];
}

// the launch of a plan (whole map or region) over `in` into `out`, workgroup by workgroup; counts as the kernel's
void run_plan(const Program& p, const W::Plan& pl, int edge, bool empty, const float* in, int rows, int cols, std::vector<float>& out,
              unsigned long long counts[2], long* bad) {
  const int m = pl.m;
  for (unsigned t = 0; t < pl.tiles; ++t) {
    int i0, j0;
    W::cell_of(pl, t, 0, &i0, &j0);
    std::vector<float> T;
    At at{in, nullptr, rows, cols, i0 - m, j0 - m, pl.tile_rows, pl.tile_cols, NAN, bad};
    if (pl.tile_in_lds) {
      T.resize((size_t)pl.tile_rows * pl.tile_cols);
      for (size_t k = 0; k < T.size(); ++k) {
        const int row = at.ia + (int)(k % pl.tile_rows), col = at.ja + (int)(k / pl.tile_rows);
        const bool inside = row >= 0 && row < rows && col >= 0 && col < cols;
        T[k] = inside ? in[(size_t)col * rows + row] : NAN;
      }
      at.tile = &T;
    }
    const bool sep = pl.route == W::kRouteSeparable && W::wg_separable(edge, m, rows, cols, i0, j0);
    ++counts[sep ? 0 : 1];
    std::vector<Partial> part;
    const int n_items = W::kTI * pl.tile_cols;
    if (sep) {
      part.assign((size_t)p.n_red * n_items, partial_empty());
      const bool clip = edge == W::kInside || edge == W::kCrop;
      Stack st;
      Res res;
      for (int item = 0; item < n_items; ++item) {
        const int row = i0 + item % W::kTI, col = j0 - m + item / W::kTI;
        if (row >= rows || (clip && (col < 0 || col >= cols))) continue;
        const int rlo = clip && row - m < 0 ? 0 : row - m, rhi = clip && row + m > rows - 1 ? rows - 1 : row + m;
        for (int r = 0; r < p.n_red; ++r) part[(size_t)r * n_items + item] = window_column(p, r, st, res, at, col, rlo, rhi);
      }
    }
    for (int lane = 0; lane < W::kThreads; ++lane) {
      int i, j;
      if (!W::cell_of(pl, t, lane, &i, &j)) continue;
      if (i < 0 || i >= rows || j < 0 || j >= cols) {  // an owned cell outside the map: no plan may say so
        ++*bad;
        continue;
      }
      float v;
      if (!sep) {
        v = direct_cell(p, edge, empty, m, at, i, j);
      } else {
        const int ii = lane % W::kTI;
        const W::Extent e = W::extent(edge, m, rows, cols, i, j, finite_f(at(i, j)), empty);
        v = NAN;
        if (e.visited) {
          Stack st;
          Res res;
          for (int r = 0; r < p.n_red; ++r) {
            Partial acc = partial_empty();
            for (int col = e.clo; col <= e.chi; ++col) partial_merge(acc, part[(size_t)r * n_items + (size_t)(col - (j0 - m)) * W::kTI + ii]);
            res.r[r] = partial_result(acc, p.red_kind[r], (uint64_t)(e.rhi - e.rlo + 1) * (uint64_t)(e.chi - e.clo + 1));
          }
          const WindowSource<Res> src{0.0f, &res};
          v = run<1>(p, 0, p.n_main, st, src).v[0];
        }
      }
      out[(size_t)j * rows + i] = v;
    }
  }
}

// one rectangle of one map and one window: out_rect, ownership, the staged extent
void check_plan(int rows, int cols, int w, const R::Rect& dirty, int option) {
  const W::RegionPlan p = W::region_plan(rows, cols, w, 1, 0, option, dirty);
  const int m = (w - 1) / 2;
  const R::Rect want = {dirty.i0 - m < 0 ? 0 : dirty.i0 - m, dirty.j0 - m < 0 ? 0 : dirty.j0 - m, dirty.i1 + m > rows ? rows : dirty.i1 + m,
                        dirty.j1 + m > cols ? cols : dirty.j1 + m};
  bool ok = p.reach == m && p.out.i0 == want.i0 && p.out.j0 == want.j0 && p.out.i1 == want.i1 && p.out.j1 == want.j1;
  ok = ok && p.k.region == 1 && p.k.oi0 == want.i0 && p.k.oj0 == want.j0 && p.k.oi1 == want.i1 && p.k.oj1 == want.j1;
  check(ok, "out_rect is the clamped growth");
  const W::Plan whole = W::plan(rows, cols, w, 1, 0, option);
  check(p.k.route == whole.route && p.k.lds_bytes == whole.lds_bytes && p.k.tile_in_lds == whole.tile_in_lds && p.k.tiles <= whole.tiles && p.k.fits == whole.fits,
        "route, LDS and staging are the whole-map plan's");
  check(p.k.tiles == (unsigned long long)((R::height(p.out) + W::kTI - 1) / W::kTI) * (unsigned long long)((R::width(p.out) + W::kTJ - 1) / W::kTJ), "the tile count");
  // ownership: every cell of out_rect exactly once, none outside
  std::vector<int> owners((size_t)rows * cols, 0);
  bool outside = false, round_trip = true, staged_ok = true;
  for (unsigned t = 0; t < p.k.tiles; ++t) {
    int i0, j0;
    W::cell_of(p.k, t, 0, &i0, &j0);
    const R::Rect st = W::staged(p.k, t);
    for (int lane = 0; lane < W::kThreads; ++lane) {
      int i, j;
      if (!W::cell_of(p.k, t, lane, &i, &j)) continue;
      if (i < p.out.i0 || i >= p.out.i1 || j < p.out.j0 || j >= p.out.j1) {
        outside = true;
        continue;
      }
      ++owners[(size_t)j * rows + i];
      unsigned t2;
      int l2;
      W::owner_of(p.k, i, j, &t2, &l2);
      round_trip = round_trip && t2 == t && l2 == lane;
      // the window of an owned cell lies in what the workgroup stages
      staged_ok = staged_ok && i - m >= st.i0 && i + m < st.i1 && j - m >= st.j0 && j + m < st.j1;
    }
    // ... and what it stages of the MAP lies in what the call may read: out grown by m, plus the rest of a border tile,
    // every index of which the staging loop and At check against the map before they load
    staged_ok = staged_ok && st.i0 == i0 - m && st.j0 == j0 - m && R::height(st) == W::kTI + 2 * m && R::width(st) == W::kTJ + 2 * m;
  }
  bool once = !outside;
  for (int j = 0; j < cols; ++j)
    for (int i = 0; i < rows; ++i) {
      const bool in_out = i >= p.out.i0 && i < p.out.i1 && j >= p.out.j0 && j < p.out.j1;
      once = once && owners[(size_t)j * rows + i] == (in_out ? 1 : 0);
    }
  check(once, "every cell of out_rect has exactly one owner and no other cell has one");
  check(round_trip, "owner_of inverts cell_of");
  check(staged_ok, "the windows of a workgroup's cells lie in its staged extent");
  const R::Rect reads = W::window_reads(p, rows, cols);
  check(R::inside(p.out, reads) && reads.i0 >= 0 && reads.j0 >= 0 && reads.i1 <= rows && reads.j1 <= cols, "the cells read lie in the map");
}

void self_checks() {
  const int windows[] = {1, 3, 5, 9, 21};
  for (int rows = 1; rows <= 12; ++rows)
    for (int cols = 1; cols <= 9; ++cols)
      for (int w : windows)
        for (int i0 = 0; i0 < rows; ++i0)
          for (int i1 = i0 + 1; i1 <= rows; ++i1)
            for (int j0 = 0; j0 < cols; ++j0)
              for (int j1 = j0 + 1; j1 <= cols; ++j1) check_plan(rows, cols, w, R::Rect{i0, j0, i1, j1}, (i0 + j1) % 3);
  std::mt19937 rng(11);
  for (int n = 0; n < 400; ++n) {
    const int rows = 70, cols = 45;
    const int i0 = (int)(rng() % rows), j0 = (int)(rng() % cols);
    const int i1 = i0 + 1 + (int)(rng() % (rows - i0)), j1 = j0 + 1 + (int)(rng() % (cols - j0));
    check_plan(rows, cols, windows[n % 5], R::Rect{i0, j0, i1, j1}, n % 3);
  }
  // the named rectangle of the GPU test: it straddles a 32-row and an 8-column seam of the WHOLE-map tiling
  check(29 / W::kTI != (29 + 7 - 1) / W::kTI && 6 / W::kTJ != (6 + 5 - 1) / W::kTJ, "(29, 6, 7, 5) straddles both seams");
  // the whole-map plan has the origin (0, 0) and the map as its end: the overloads agree with the old ones
  const W::Plan whole = W::plan(70, 45, 5, 1, 0, 0);
  check(whole.region == 0 && whole.oi0 == 0 && whole.oj0 == 0 && whole.oi1 == 70 && whole.oj1 == 45, "the whole-map plan owns the map");
  bool same = true;
  for (unsigned t = 0; t < whole.tiles; ++t)
    for (int lane = 0; lane < W::kThreads; lane += 37) {
      int a, b, c, d;
      W::cell_of(whole.tiles_i, t, lane, &a, &b);
      const bool mine = W::cell_of(whole, t, lane, &c, &d);
      same = same && a == c && b == d && mine == (a < 70 && b < 45);
    }
  check(same, "cell_of(plan) of the whole-map plan is cell_of(tiles_i)");
  // nothing is sized by the map
  const W::RegionPlan big = W::region_plan(8192, 8192, 21, 1, 0, 0, R::Rect{4000, 4000, 4256, 4256});
  const W::RegionPlan small = W::region_plan(2048, 2048, 21, 1, 0, 0, R::Rect{1000, 1000, 1256, 1256});
  check(big.k.tiles == small.k.tiles && big.k.tiles == 9ull * 35ull && big.k.lds_bytes == small.k.lds_bytes, "276 x 276 cells: 9 x 35 tiles on either map");
  check(!W::plan(64, 64, W::smallest_window_off_lds(), 1, 0, 0).tile_in_lds && W::plan(64, 64, W::smallest_window_off_lds() - 2, 1, 0, 0).tile_in_lds,
        "smallest_window_off_lds is the threshold");
}

std::vector<float> read_floats(const char* path, size_t n) {
  std::vector<float> v(n);
  FILE* f = fopen(path, "rb");
  if (!f || fread(v.data(), sizeof(float), n, f) != n) {
    fprintf(stderr, "window_region_check: cannot read %zu floats from %s\n", n, path);
    exit(2);
  }
  fclose(f);
  return v;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 1) {
    self_checks();
    printf("%d checks, %d failed checks\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
  }
  const std::string mode = argv[1];
  if (mode == "offlds" && argc == 2) {
    printf("%d\n", W::smallest_window_off_lds());
    return 0;
  }
  if (mode == "plan" && argc == 12) {
    const int rows = atoi(argv[2]), cols = atoi(argv[3]), w = atoi(argv[4]), n_red = atoi(argv[5]), n_outer = atoi(argv[6]), option = atoi(argv[7]);
    const int r0 = atoi(argv[8]), c0 = atoi(argv[9]), h = atoi(argv[10]), wd = atoi(argv[11]);
    if (rows < 1 || cols < 1 || w < 1 || w % 2 == 0 || !R::valid_rect(rows, cols, r0, c0, h, wd)) return 2;
    const W::RegionPlan p = W::region_plan(rows, cols, w, n_red, n_outer, option, R::Rect{r0, c0, r0 + h, c0 + wd});
    printf("%s %d %d %d %d %d %llu %d\n", p.k.route == W::kRouteSeparable ? "separable" : "direct", p.reach, p.out.i0, p.out.j0, R::height(p.out), R::width(p.out),
           p.k.tiles, p.k.tile_in_lds);
    return 0;
  }
  if (mode != "eval" || argc != 17) {
    fprintf(stderr, "usage: window_region_check [plan ... | offlds | eval TEXT LAYER ROWS COLS W EDGE EMPTY OPTION ROW0 COL0 H WD IN.bin PREV.bin OUT.bin]\n");
    return 2;
  }
  Program p;
  char err[256];
  if (compile_window(argv[2], atoi(argv[3]), &p, err, sizeof(err)) != kOk) {
    printf("ERR %s\n", err);
    return 0;
  }
  const int rows = atoi(argv[4]), cols = atoi(argv[5]), w = atoi(argv[6]), edge = atoi(argv[7]), empty = atoi(argv[8]), option = atoi(argv[9]);
  const int r0 = atoi(argv[10]), c0 = atoi(argv[11]), h = atoi(argv[12]), wd = atoi(argv[13]);
  if (rows < 1 || cols < 1 || w < 1 || w % 2 == 0 || edge < 0 || edge > 3 || !R::valid_rect(rows, cols, r0, c0, h, wd)) return 2;
  const std::vector<float> in = read_floats(argv[14], (size_t)rows * cols);
  std::vector<float> out = read_floats(argv[15], (size_t)rows * cols);
  const W::RegionPlan plan = W::region_plan(rows, cols, w, p.n_red, p.n_outer, option, R::Rect{r0, c0, r0 + h, c0 + wd});
  unsigned long long counts[2] = {0, 0}, expected[2];
  long bad = 0;
  run_plan(p, plan.k, edge, empty != 0, in.data(), rows, cols, out, counts, &bad);
  W::expected_counts(plan.k, edge, rows, cols, expected);
  if (expected[0] != counts[0] || expected[1] != counts[1]) ++bad;
  FILE* f = fopen(argv[16], "wb");
  if (!f || fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) return 2;
  fclose(f);
  printf("OK %d %d %d %d %llu %llu %ld\n", plan.out.i0, plan.out.j0, R::height(plan.out), R::width(plan.out), counts[0], counts[1], bad);
  return 0;
}
