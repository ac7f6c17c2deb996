// CPU harness of te_move_plan.h and of the transition te::CtxState::map_moved (tests/test_move_plan.py):
//   sweep          every shift from -(n + 2) to n + 2 on both axes for maps of 1 x 1 up to 12 x 9: the exposed rectangles are
//                  disjoint and cover exactly the cells whose source lies outside the old window, the trailing lines are the
//                  opposite border lines of the axes that moved; one line per plan for the comparison with the numpy reference
//   round          requested shifts of a fraction of a cell, from several held positions and resolutions
//   ties           results_kept for the default parameters at 0.05 m and 0.03 m, tie-free radii, and raster normals
//   state          map_moved(true / false) from the states a walk over the other transitions reaches
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "te_ctx_state.h"
#include "te_move_plan.h"

namespace {

int g_failed = 0;
#define CHECK(cond, ...)                     \
  do {                                       \
    if (!(cond)) {                           \
      if (++g_failed <= 20) {                \
        printf("FAILED %s: ", #cond);        \
        printf(__VA_ARGS__);                 \
        printf("\n");                        \
      }                                      \
    }                                        \
  } while (0)

te_params default_params() {  // te_params_default (te_shim.hip)
  te_params p;
  memset(&p, 0, sizeof(p));
  p.size = (uint32_t)sizeof(p);
  p.abi_version = TE_ABI_VERSION;
  p.normals_radius = 0.05, p.normals_axis = 2, p.slope_critical = 1.0;
  p.step_critical = 0.12, p.step_radius1 = 0.04, p.step_radius2 = 0.04, p.step_ncrit = 4;
  p.rough_critical = 0.05, p.rough_radius = 0.05;
  p.w_scale = 1.0f / 3.0f, p.w_slope = p.w_step = p.w_rough = 1.0f;
  p.fp_radius = 0.30, p.fp_offset = 0.15, p.fp_default = 0.3, p.fp_max_gap = 0.3, p.fp_critical_step = 0.12;
  return p;
}
te_params tie_free_params(double res) {  // synth.benchmark_radius(5, res) everywhere
  te_params p = default_params();
  const double r = 5.0 * res * (1.0 + 1e-6);
  p.normals_radius = p.rough_radius = p.step_radius1 = p.step_radius2 = p.fp_radius = r;
  p.fp_offset = 0.0;
  return p;
}

int sweep() {
  const te_params tf = tie_free_params(1.0);
  long long plans = 0;
  for (int rows = 1; rows <= 12; ++rows)
    for (int cols = 1; cols <= 9; ++cols)
      for (int kr = -(rows + 2); kr <= rows + 2; ++kr)
        for (int kc = -(cols + 2); kc <= cols + 2; ++kc, ++plans) {
          te::move::Plan p;
          const char* why = "";
          const int rc = te::move::plan(rows, cols, 1.0, 0.0, 0.0, (double)kr, (double)kc, &tf, false, &p, &why);
          const te_move_info& m = p.info;
          CHECK(rc == TE_OK, "%dx%d (%d,%d): %s", rows, cols, kr, kc, why);
          CHECK(m.shift_rows == kr && m.shift_cols == kc && m.pos_x == (double)kr && m.pos_y == (double)kc, "%dx%d (%d,%d): shift (%d,%d)", rows,
                cols, kr, kc, m.shift_rows, m.shift_cols);
          CHECK(m.results_kept == 1, "%dx%d (%d,%d)", rows, cols, kr, kc);
          // cover[j * rows + i]: how many exposed rectangles hold the cell
          std::vector<int> cover((size_t)rows * cols, 0);
          int n_exposed = 0, n_lines = 0;
          for (int k = 0; k < m.n_rects; ++k) {
            const int* r = m.rects[k];
            CHECK(r[0] >= 0 && r[1] >= 0 && r[2] > 0 && r[3] > 0 && r[2] <= rows - r[0] && r[3] <= cols - r[1], "%dx%d (%d,%d): rect %d outside", rows,
                  cols, kr, kc, k);
            if (!m.rect_exposed[k]) {
              ++n_lines;
              continue;
            }
            CHECK(n_lines == 0, "%dx%d (%d,%d): an exposed rectangle behind a line", rows, cols, kr, kc);
            ++n_exposed;
            for (int j = r[1]; j < r[1] + r[3]; ++j)
              for (int i = r[0]; i < r[0] + r[2]; ++i) cover[(size_t)j * rows + i]++;
          }
          bool all = true;
          for (int j = 0; j < cols; ++j)
            for (int i = 0; i < rows; ++i) {
              const bool outside = i - kr < 0 || i - kr >= rows || j - kc < 0 || j - kc >= cols;
              all = all && outside;
              CHECK(cover[(size_t)j * rows + i] == (outside ? 1 : 0), "%dx%d (%d,%d): cell (%d,%d) in %d exposed rectangles", rows, cols, kr, kc, i, j,
                    cover[(size_t)j * rows + i]);
              // the kernel's ranges say the same (a plan without a launch has none)
              const bool has_src = i >= p.i_lo && i < p.i_hi && j >= p.j_lo && j < p.j_hi;
              CHECK(p.scratch_bytes == 0 || has_src == !outside,"%dx%d (%d,%d): cell (%d,%d) source range", rows, cols, kr, kc, i, j);
            }
          const bool zero = kr == 0 && kc == 0;
          CHECK((m.all_exposed != 0) == (all && !zero), "%dx%d (%d,%d): all_exposed %d", rows, cols, kr, kc, m.all_exposed);
          CHECK(n_exposed <= 2 && n_lines <= 2, "%dx%d (%d,%d)", rows, cols, kr, kc);
          if (zero) CHECK(m.n_rects == 0 && p.scratch_bytes == 0, "zero shift");
          if (m.all_exposed) {
            CHECK(m.n_rects == 1 && n_lines == 0 && p.scratch_bytes == 0, "%dx%d (%d,%d): all exposed", rows, cols, kr, kc);
          } else if (!zero) {
            // trailing lines: the border opposite to the exposed band, on the axes that moved and on no other
            int want_lines = 0, k = n_exposed;
            if (kr != 0) {
              const int* r = m.rects[k++];
              ++want_lines;
              CHECK(r[0] == (kr > 0 ? rows - 1 : 0) && r[1] == 0 && r[2] == 1 && r[3] == cols, "%dx%d (%d,%d): row line", rows, cols, kr, kc);
            }
            if (kc != 0) {
              const int* r = m.rects[k++];
              ++want_lines;
              CHECK(r[0] == 0 && r[1] == (kc > 0 ? cols - 1 : 0) && r[2] == rows && r[3] == 1, "%dx%d (%d,%d): column line", rows, cols, kr, kc);
            }
            CHECK(n_lines == want_lines && k == m.n_rects, "%dx%d (%d,%d): %d lines", rows, cols, kr, kc, n_lines);
            CHECK(p.scratch_bytes == (size_t)rows * cols * sizeof(float) && p.grid_x >= 1 && p.grid_y >= 1, "%dx%d (%d,%d): launch", rows, cols, kr, kc);
            CHECK((long long)p.grid_x * te::move::kLanes >= (rows >> 2) + 2 || p.grid_x == te::move::kMaxGridX, "grid_x");
            CHECK((long long)p.grid_y * te::move::kCols >= cols || p.grid_y == te::move::kMaxGridY, "grid_y");
          }
          printf("plan %d %d %d %d %d %d", rows, cols, kr, kc, m.n_rects, m.all_exposed);
          for (int q = 0; q < m.n_rects; ++q) printf(" %d,%d,%d,%d,%d", m.rects[q][0], m.rects[q][1], m.rects[q][2], m.rects[q][3], m.rect_exposed[q]);
          printf("\n");
        }
  printf("%lld plans, %d failed checks\n", plans, g_failed);
  return g_failed ? 1 : 0;
}

// round HELD_X HELD_Y RES: one line per requested fraction of a cell, on x and (negated) on y
int rounding(double hx, double hy, double res) {
  const double frac[] = {0.0, 0.49, -0.49, 0.5, -0.5, 1.5, -1.5, 2.49, -7.5, 1e-9, 300.5};
  for (double f : frac) {
    te::move::Plan p;
    const char* why = "";
    const double nx = hx + f * res, ny = hy - f * res;
    if (te::move::plan(40, 30, res, hx, hy, nx, ny, nullptr, false, &p, &why) != TE_OK) return 1;
    // the bits of the positions, so that "bit-identical" is checked as such
    unsigned long long bx, by;
    memcpy(&bx, &p.info.pos_x, 8);
    memcpy(&by, &p.info.pos_y, 8);
    printf("round %.17g %.17g %d %d %llx %llx %d\n", nx, ny, p.info.shift_rows, p.info.shift_cols, bx, by, p.info.n_rects);
  }
  return 0;
}

int ties() {
  struct Case {
    const char* name;
    te_params p;
    double res;
    bool raster, no_params;
  };
  te_params big = tie_free_params(0.05);
  big.fp_radius = 25.0 * 0.05 * (1.0 + 1e-6);  // a reach above 20 cells, tie-free
  te_params fp_tie = tie_free_params(0.05);
  fp_tie.fp_offset = 0.25 - fp_tie.fp_radius + 0.25;  // radius + offset = 10 cells exactly
  const Case cases[] = {{"default_0.05", default_params(), 0.05, false, false}, {"default_0.03", default_params(), 0.03, false, false},
                        {"tie_free_0.05", tie_free_params(0.05), 0.05, false, false}, {"tie_free_0.03", tie_free_params(0.03), 0.03, false, false},
                        {"tie_free_raster", tie_free_params(0.05), 0.05, true, false}, {"tie_free_reach_25", big, 0.05, false, false},
                        {"footprint_tie_only", fp_tie, 0.05, false, false}, {"no_params", default_params(), 0.05, false, true}};
  for (const Case& c : cases) {
    te::move::Plan p;
    const char* why = "";
    if (te::move::plan(64, 48, c.res, 1.0, 2.0, 1.0 + 3 * c.res, 2.0, c.no_params ? nullptr : &c.p, c.raster, &p, &why) != TE_OK) return 1;
    printf("ties %s %d\n", c.name, p.info.results_kept);
  }
  // bad arguments
  te::move::Plan p;
  const char* why = "";
  const double nan = __builtin_nan(""), inf = __builtin_inf();
  printf("args %d %d %d %d %d\n", te::move::plan(4, 4, 0.05, 0, 0, nan, 0, nullptr, false, &p, &why), te::move::plan(4, 4, 0.05, 0, 0, 0, inf, nullptr, false, &p, &why),
         te::move::plan(0, 4, 0.05, 0, 0, 0, 0, nullptr, false, &p, &why), te::move::plan(4, 4, 0.0, 0, 0, 0, 0, nullptr, false, &p, &why),
         te::move::plan(4, 4, 0.05, nan, 0, 0, 0, nullptr, false, &p, &why));
  return 0;
}

// a walk over the other transitions (the entry points of tests/cpu/ctx_state_check.cpp's sweep, with their refusals)
int state(int n_seq, unsigned seed) {
  using te::CtxState;
  std::mt19937 rng(seed);
  auto pick = [&rng](unsigned n) { return (unsigned)(rng() % n); };
  long long steps = 0, kept_with_results = 0;
  for (int q = 0; q < n_seq; ++q) {
    CtxState s;
    const int len = 1 + (int)pick(30);
    for (int k = 0; k < len; ++k, ++steps) {
      const unsigned flags = pick(64);
      switch (pick(13)) {
        case 0: s.geometry_set(); break;
        case 1: s.elevation_replaced(); if (pick(4)) s.elevation_counted(pick(100), pick(100), 0.07); break;
        case 2: s.elevation_tile_written(); break;
        case 3: s.layer_touched(TE_LAYER_ELEVATION); s.elevation_pointer_out(); break;
        case 4: { const int layer = 1 + (int)pick(TE_LAYER_COUNT - 1); s.layer_touched(layer); s.layer_written(layer, pick(2) ? CtxState::kUploaded : CtxState::kPointerOut); break; }
        case 5: s.prefetch_joined(pick(1u << TE_LAYER_COUNT), pick(3) != 0); break;
        case 6: s.params_changed(pick(2) != 0, pick(2) != 0, pick(4) == 0); break;
        case 7: case 8: if (s.have_elev()) s.graph_replayed(flags & ~TE_RUN_NORMALS_ONLY); break;
        case 9: if (s.chain_done()) s.footprint_launched(true); break;
        case 10: if (s.chain_done()) { const bool m = s.mask_done(); s.chain_launching(false, 0); s.chain_launched(false, 0); if (s.footprint_done() && pick(2)) s.region_footprint_refreshed(m); } break;
        case 11: if (s.have_elev()) s.filter_ran(TE_FILTER_SLOPE + (int)pick(5)); break;
        case 12: if (s.chain_done() && !s.mask_done()) s.mask_built(); break;
      }
      // results kept: the region contract -- these stay ...
      CtxState a = s;
      a.map_moved(true);
      CHECK(a.have_elev() == s.have_elev() && a.chain_done() == s.chain_done() && a.footprint_done() == s.footprint_done() &&
                a.layers_written() == s.layers_written() && a.have_robot_slope() == s.have_robot_slope() && a.trav_external() == s.trav_external() &&
                a.trav_ptr_out() == s.trav_ptr_out() && a.combine_deferred() == s.combine_deferred() && a.elev_ptr_out() == s.elev_ptr_out(),
            "map_moved(true) changed a fact of the region contract");
      // ... and these go: the count, the face flags, the mask
      CHECK(a.invalid_cells() == -1 && a.invalid_runs() == -1 && a.face_crit() != a.face_crit() && !a.mask_done() && !a.face_flags_for(0.07, 0.07),
            "map_moved(true) kept the count, the face flags or the mask");
      CtxState t = s;  // ... which is a tile upload plus the mask
      t.elevation_tile_written();
      CHECK(!s.have_elev() || a.have_elev() == t.have_elev(), "have_elev");
      kept_with_results += a.chain_done() && a.footprint_done();
      // results dropped: a whole upload
      CtxState b = s, e = s;
      b.map_moved(false);
      e.elevation_replaced();
      CHECK(b == e, "map_moved(false) is not elevation_replaced()");
      CHECK(!b.chain_done() && !b.footprint_done() && !b.mask_done() && b.have_elev(), "map_moved(false) kept a result");
    }
  }
  printf("%d sequences, %lld steps, %lld with chain and footprint kept, %d failed checks\n", n_seq, steps, kept_with_results, g_failed);
  return g_failed ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "sweep")) return sweep();
  if (argc >= 5 && !strcmp(argv[1], "round")) return rounding(atof(argv[2]), atof(argv[3]), atof(argv[4]));
  if (argc >= 2 && !strcmp(argv[1], "ties")) return ties();
  if (argc >= 4 && !strcmp(argv[1], "state")) return state(atoi(argv[2]), (unsigned)atoi(argv[3]));
  fprintf(stderr, "usage: move_plan_check sweep | round HX HY RES | ties | state N SEED\n");
  return 2;
}
