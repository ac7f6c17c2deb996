// CPU harness over te_window_plan.h, the plan of te_run_window_expression (tests/test_window_plan.py).
//   window_plan_check                                     the built-in checks -> "N checks, F failed checks"
//   window_plan_check size WINDOW_SIZE USE_LENGTH LENGTH RESOLUTION   -> "w" | "ERR reason"
//   window_plan_check route ROWS COLS W EDGE N_RED N_OUTER OPTION     -> "separable|direct tile_in_lds lds_bytes count_separable count_direct"
//   window_plan_check offlds                              -> the smallest odd window whose tile the plan does not stage in LDS
// Build: g++ -std=c++17 -O2.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "te_window_plan.h"

using namespace te::wexpr;

namespace {

int g_checks = 0, g_failed = 0;
void check(bool ok, const char* what) {
  ++g_checks;
  if (!ok) {
    ++g_failed;
    printf("FAILED: %s\n", what);
  }
}

int size_of(int ws, int use, double len, double res) {
  int w = -1;
  return window_from_params(ws, use, len, res, &w) ? -1 : w;
}

void self_checks() {
  // rule 2
  check(size_of(0, 1, 0.05, 0.03) == 3 && size_of(0, 1, 0.1, 0.05) == 3 && size_of(0, 1, 0.15, 0.05) == 3, "lengths that give 3");
  check(size_of(0, 1, 0.025, 0.05) == 1 && size_of(0, 1, 0.02, 0.05) == 1 && size_of(0, 1, 0.25, 0.05) == 5 && size_of(0, 1, 0.0, 0.05) == 1, "lengths that give 1 and 5");
  check(size_of(0, 1, -0.1, 0.05) == -1 && size_of(0, 1, NAN, 0.05) == -1 && size_of(0, 1, INFINITY, 0.05) == -1 && size_of(0, 1, 1.0e12, 0.05) == -1, "bad lengths");
  check(size_of(5, 0, 0.0, 0.05) == 5 && size_of(4, 0, 0.0, 0.05) == -1 && size_of(0, 0, 0.0, 0.05) == -1 && size_of(-3, 0, 0.0, 0.05) == -1, "window_size as given");

  // every cell of a map has exactly one owner, and the owner's cell is that cell
  for (const auto& shape : {std::pair<int, int>{5, 7}, {70, 37}, {130, 33}, {32, 8}, {33, 9}, {1, 1}}) {
    const int rows = shape.first, cols = shape.second;
    const Plan p = plan(rows, cols, 5, 1, 0, 0);
    std::vector<int> owners((size_t)rows * cols, 0);
    bool beyond = false;
    for (unsigned t = 0; t < p.tiles; ++t)
      for (int lane = 0; lane < kThreads; ++lane) {
        int i, j;
        cell_of(p.tiles_i, t, lane, &i, &j);
        if (i < 0 || j < 0) beyond = true;
        if (i >= rows || j >= cols) continue;
        ++owners[(size_t)j * rows + i];
        unsigned t2;
        int lane2;
        owner_of(p.tiles_i, i, j, &t2, &lane2);
        if (t2 != t || lane2 != lane) beyond = true;
      }
    bool once = !beyond;
    for (int n : owners) once = once && n == 1;
    check(once, "exactly one owner per cell");
    check(p.tiles == (unsigned long long)((rows + kTI - 1) / kTI) * ((cols + kTJ - 1) / kTJ), "the tile count");
  }

  // tile + halo and the column partials never exceed the LDS figure; what is staged covers every read of the workgroup
  for (int w = 1; w <= 301; w += 2)
    for (int n_red = 0; n_red <= 4; ++n_red)
      for (int option = 0; option <= 2; ++option) {
        const Plan p = plan(200, 100, w, n_red, 0, option);
        check(p.lds_bytes <= kMaxLds, "LDS within the figure");
        check(p.off_tile == kBaseLds && p.off_part % sizeof(double) == 0, "offsets");
        if (p.tile_in_lds) check(p.off_part - p.off_tile == (size_t)p.tile_rows * p.tile_cols * sizeof(float) && p.tile_rows == kTI + 2 * p.m && p.tile_cols == kTJ + 2 * p.m, "the staged tile");
        if (p.route == kRouteSeparable)
          check(p.tile_in_lds && n_red > 0 && option != 2 && p.lds_bytes == p.off_part + (size_t)n_red * kTI * p.tile_cols * kPartialBytes, "the column partials");
        if (option == 2) check(p.route == kRouteDirect, "option 2 is the direct route");
        if (option == 0 && w < kSepMinWindow) check(p.route == kRouteDirect, "by plan a window below kSepMinWindow walks directly");
      }
  const int off = smallest_window_off_lds();
  check(off > 21 && plan(64, 64, off, 1, 0, 0).tile_in_lds == 0 && plan(64, 64, off - 2, 1, 0, 0).tile_in_lds == 1 && plan(64, 64, off, 1, 0, 1).route == kRouteDirect,
        "the smallest window off LDS");
  check(plan(64, 64, 2147483647, 1, 0, 0).fits && plan(64, 64, 2147483647, 1, 0, 0).tile_in_lds == 0, "the largest window is served from global memory");

  // route eligibility
  check(plan(70, 37, 5, 3, 1, 0).route == kRouteDirect && plan(70, 37, 5, 3, 1, 1).route == kRouteDirect, "nested -> direct");
  check(plan(70, 37, 5, 1, 0, 0).route == kRouteSeparable && plan(70, 37, 9, 4, 0, 0).route == kRouteSeparable, "not nested, w >= 5 -> separable");
  check(plan(70, 37, 3, 1, 0, 0).route == kRouteDirect && plan(70, 37, 3, 1, 0, 1).route == kRouteSeparable, "w = 3: by plan direct, forced separable");
  check(plan(70, 37, 1, 1, 0, 0).route == kRouteDirect && plan(70, 37, 1, 1, 0, 1).route == kRouteSeparable, "w = 1: by plan direct, forced separable");
  check(plan(70, 37, 5, 0, 0, 1).route == kRouteDirect, "no reduction -> direct");
  // `mean` padding: only a workgroup none of whose windows is clipped is separable
  check(!wg_separable(kMean, 2, 200, 100, 0, 0) && wg_separable(kMean, 2, 200, 100, 32, 8) && !wg_separable(kMean, 2, 200, 100, 192, 8) &&
            !wg_separable(kMean, 2, 200, 100, 32, 96) && wg_separable(kMean, 2, 200, 100, 160, 88),
        "mean: clipped workgroups walk directly");
  check(wg_separable(kMean, 2, 70, 37, 32, 8) && !wg_separable(kMean, 2, 70, 37, 64, 8), "mean: the last partial tile is judged by the cells it has");
  check(wg_separable(kCrop, 2, 200, 100, 0, 0) && wg_separable(kEmpty, 2, 200, 100, 0, 0) && wg_separable(kInside, 2, 200, 100, 0, 0), "the other edge handlings: every workgroup");

  // rule 3
  {
    Extent e = extent(kCrop, 2, 10, 8, 0, 7, true, true);
    check(e.visited && e.clipped && e.rlo == 0 && e.rhi == 2 && e.clo == 5 && e.chi == 7, "crop at a corner");
    e = extent(kEmpty, 2, 10, 8, 0, 7, true, true);
    check(e.visited && e.rlo == -2 && e.rhi == 2 && e.clo == 5 && e.chi == 9 && e.blo == 0 && e.bchi == 7, "empty at a corner");
    check(!extent(kInside, 2, 10, 8, 1, 4, true, true).visited && extent(kInside, 2, 10, 8, 2, 5, true, true).visited && !extent(kInside, 2, 10, 8, 2, 6, true, true).visited,
          "inside");
    check(!extent(kCrop, 2, 10, 8, 4, 4, false, false).visited && extent(kCrop, 2, 10, 8, 4, 4, false, true).visited, "compute_empty_cells");
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 1) {
    self_checks();
    printf("%d checks, %d failed checks\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
  }
  const std::string mode = argv[1];
  if (mode == "size" && argc == 6) {
    int w = 0;
    const char* why = window_from_params(atoi(argv[2]), atoi(argv[3]), atof(argv[4]), atof(argv[5]), &w);
    if (why)
      printf("ERR %s\n", why);
    else
      printf("%d\n", w);
    return 0;
  }
  if (mode == "route" && argc == 9) {
    const int rows = atoi(argv[2]), cols = atoi(argv[3]), edge = atoi(argv[5]);
    const Plan p = plan(rows, cols, atoi(argv[4]), atoi(argv[6]), atoi(argv[7]), atoi(argv[8]));
    unsigned long long counts[2];
    expected_counts(p, edge, rows, cols, counts);
    printf("%s %d %zu %llu %llu\n", p.route == kRouteSeparable ? "separable" : "direct", p.tile_in_lds, p.lds_bytes, counts[0], counts[1]);
    return 0;
  }
  if (mode == "offlds" && argc == 2) {
    printf("%d\n", smallest_window_off_lds());
    return 0;
  }
  fprintf(stderr, "usage: window_plan_check [size WS USE LEN RES | route ROWS COLS W EDGE N_RED N_OUTER OPTION | offlds]\n");
  return 2;
}
