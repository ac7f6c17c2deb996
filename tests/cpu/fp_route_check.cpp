// fp_route_check.cpp -- the route of the circular footprint pass from the header launch_footprint routes
// with (te_fp_route.h), on the disc of te_disc.h and the spiral of te_fp_table.h (the tables the shim builds).  tests/test_fp_route.py.
//   fp_route_check cases         one line per named case: "name route k strip_rows chunk blocked"
//   fp_route_check sweep N SEED  N seeded cases; every route is held to what its kernels rely on: "N cases, F failed checks"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "te_disc.h"
#include "te_fp_route.h"
#include "te_fp_table.h"

using namespace te;
using namespace te::fast;

static const char* kRouteName[] = {"slide5", "slide4", "slide3", "general", "any"};

struct Case {
  double rmax_cells, rmin_cells;  // radiusMax and radiusMin in cells
  int rows, cols, batch;
  double tcap = (double)(1.0f / 3.0f) * 3.0;  // the default weights: a layer the chain wrote
  double def = 0.3;
  int cus = 256;
  bool opt_any = false;  // TE_OPT_FP_ANY_REACH
  bool region = false;   // the grown region of a region run: [i0, i1) x [j0, j1) of one map
  int i0 = 0, i1 = 0, j0 = 0, j1 = 0;
  bool guard_rows = true, has_list = true, has_scratch = true;
  double list_scale = 1.0;  // the list the shim allocates (cells + fp_list_slack), or less
};

// the route's inputs as launch_footprint fills them: the disc and its tie summary from te_disc.h, the spiral from te_fp_table.h
static FpRouteIn inputs(const Case& c) {
  const double res = 0.05;
  FpTable t;
  build_fp_table(c.rmax_cells * res, res, c.rows, c.cols, &t, false);
  FpRouteIn in;
  in.R = t.R;
  in.npoints = 0;
  in.Q = -1;
  for (int b = 0; b <= t.R; ++b)
    if (t.hw[b] >= 0) {
      in.npoints += (b == 0 ? 1 : 2) * (2 * t.hw[b] + 1);
      in.Q = t.hw[b] * t.hw[b] + b * b > in.Q ? t.hw[b] * t.hw[b] + b * b : in.Q;
    }
  in.n_ties = (int)t.ties.size() / 2;
  if (in.n_ties) in.Q = -1;  // (build_disc names tie-free shapes only)
  in.reach = t.reach;
  in.ties_on_circle = true;
  in.n_gen = 0;
  for (int k = 0; k < in.n_ties; ++k) {
    const int di = t.ties[2 * k], dj = t.ties[2 * k + 1];
    in.ties_on_circle = in.ties_on_circle && di * di + dj * dj == in.reach * in.reach;
    in.n_gen += di != 0 && dj != 0;
  }
  // Above 32 cells build_disc refuses and the shim builds no fp_disc (the route of any reach serves the pass); the cases here
  // reach further and keep the values derived from the table above.  Every other case takes them as launch_footprint does:
  Disc d;
  if (build_disc(c.rmax_cells * res, res, &d) == kDiscOk) {
    in.R = d.R;
    in.Q = d.Q;
    in.npoints = d.npoints;
    in.n_ties = d.n_ties;
    tie_summary(d, in.reach, &in.ties_on_circle, &in.n_gen);
  }
  in.n_spiral = (int)t.spiral.size();
  in.rmin = c.rmin_cells * res;
  in.def = c.def;
  in.tcap = c.tcap;
  in.rows = c.rows;
  in.cols = c.cols;
  in.batch = c.batch;
  in.region = c.region;
  in.i0 = c.region ? c.i0 : 0;
  in.i1 = c.region ? c.i1 : c.rows;
  in.j0 = c.region ? c.j0 : 0;
  in.j1 = c.region ? c.j1 : c.cols;
  in.guard_rows = c.guard_rows;
  in.has_list = c.has_list;
  in.has_scratch = c.has_scratch;
  const double cells = (double)c.rows * c.cols * c.batch;
  in.list_cap = (size_t)((cells + (double)fp_list_slack(c.rows, c.cols, c.batch, c.cus)) * c.list_scale);
  in.cus = c.cus;
  in.any = c.opt_any || in.reach > 20;  // (the shim: above 20 cells only the route of any reach has tables)
  return in;
}

// what the kernels of the route rely on; returns the number of failed checks (printed)
static int check(const FpRouteIn& in, const FpRoute& r, const char* ctx) {
  int bad = 0;
  auto req = [&](bool ok, const char* what) {
    if (!ok) {
      ++bad;
      printf("FAIL %s: %s (route %s, R %d Q %d reach %d ties %d, %d x %d x %d)\n", ctx, what, kRouteName[r.route], in.R, in.Q, in.reach,
             in.n_ties, in.rows, in.cols, in.batch);
    }
  };
  const double cells = (double)in.rows * in.cols;
  const int nbx_l = in.region ? (in.i1 - 1) / 64 - in.i0 / 64 + 1 : (in.rows + 63) / 64;
  const int H = in.region ? in.j1 - in.j0 : in.cols;
  const int nz = in.region ? 1 : in.batch;
  // The double kernels pack the untraversable count into the disc sum (one double per cell, T' + kFpUOff * U): they are
  // planned only under a bound that keeps the whole disc's |sum T'| -- and with it every |T'| -- below kFpUOff / 2.  The
  // bound is restated here from the kernels' decoding, not taken from fp_packed_ok.
  const double disc_cells = (double)in.npoints + (double)in.n_ties;
  const bool packed_bound = in.tcap >= 0.0 && disc_cells * std::fmax(in.tcap, std::fabs(in.def)) < 0.5 * kFpUOff;
  req(!in.any || r.route == kFpAny, "the route of any reach when asked for or above 20 cells");
  if (r.route == kFpSlide3 || r.route == kFpGeneral)
    req(packed_bound, "a kernel that packs the untraversable count into the sum only with npoints * cap < kFpUOff / 2");
  if (r.route == kFpAny && !in.any) req(!fp_packed_ok(disc_cells, in.tcap, in.def), "the route of any reach only for want of that bound");
  if (r.route == kFpGeneral) req(in.reach >= 1 && in.reach <= 20, "k_fp_slide<R> is instantiated for reach 1 .. 20");
  if (r.route == kFpSlide5 || r.route == kFpSlide3) {
    req(in.n_ties == 0 && in.reach == in.R, "a tie-free disc");
    req(in.rows >= 64 && in.rows >= 2 * in.R + 1 && in.cols >= 2 * in.R + 1, "a map one wavefront and one disc wide");
    req(cells * 4.0 < 4294967296.0, "32-bit byte offsets within a map");
  }
  if (r.route == kFpSlide3) {
    req(fp_f3_shape(in.Q), "the shape is instantiated (TE_F3_P*)");
    req(in.n_spiral <= ((int)(3.2 * (in.R + 1) * (in.R + 1) / 64) + 1) * 64, "the spiral fits the table registers");
  }
  if (r.route == kFpSlide5 || r.route == kFpSlide4) {
    req(r.k >= 17, "fixed point k >= 17");
    req(in.tcap >= 0.0 && in.def >= 0.0, "a bounded layer");
    req(in.has_list && cells * in.batch <= (double)in.list_cap, "one list entry per cell");
    req(r.strip_rows >= 1 && r.strip_rows <= 512, "strips of 1 .. 512 rows");
    req(r.chunk == (r.strip_rows >= 4 ? kF4Chunk : (r.strip_rows * 64 >= kF4Chunk / 2 ? kF4Chunk / 2 : 64)), "the chunk of the strip");
    req(r.blocked == (in.rmin != 0.0), "k_fp_blocked follows exactly when radiusMin > 0");
  } else {
    req(!r.blocked, "k_fp_blocked only behind the fixed-point kernels");
  }
  const int nstrips = r.strip_rows > 0 ? (H + r.strip_rows - 1) / r.strip_rows : 0;
  if (r.route == kFpSlide5) {
    req(2 * in.R + 1 <= 31, "2R+1 <= 31");
    req(fp_f5_shape(in.Q), "the shape is instantiated (TE_F5_P*)");
    req(in.has_scratch && in.guard_rows, "the scratch and the guard rows");
    req(in.npoints * (std::ldexp(1.0, r.k) * std::fmax(in.tcap, in.def) + 1.0) < (double)(1u << kF5UBit), "a disc's T-sum below the flag bit");
    req((double)nbx_l * nz * ((double)H * 64.0 + (double)nstrips * r.chunk) <= (double)in.list_cap, "the reservations fit the list");
  }
  if (r.route == kFpSlide4) {
    req(in.n_ties > 0 && in.ties_on_circle, "a whole-cell tie radius");
    req(fp_f4_shape(in.reach * in.reach), "the shape is instantiated (TE_F4_SHAPES_ALL)");
    req(in.n_gen == tie_triple_cells(in.reach) && in.n_ties == 4 + in.n_gen, "the circle's cells are the ones the kernel knows");
    req(in.rows >= 64 && in.rows >= 2 * in.reach + 1 && in.cols >= 2 * in.reach + 1, "a map one wavefront and one disc wide");
    req(cells * 4.0 < 4294967296.0, "32-bit byte offsets within a map");
    req((2 * in.reach + 1) * (std::ldexp(1.0, r.k) * std::fmax(in.tcap, in.def) + 1.0) < 16777216.0, "an edge sum below 2^24");
    req((double)nbx_l * nstrips * nz * r.chunk + cells * nz <= (double)in.list_cap, "the chunks fit the list");
  }
  return bad;
}

static void named(const char* name, const Case& c) {
  const FpRouteIn in = inputs(c);
  const FpRoute r = plan_fp_route(in);
  if (check(in, r, name)) exit(1);
  printf("%s %s %d %d %d %d\n", name, kRouteName[r.route], r.k, r.strip_rows, r.chunk, r.blocked ? 1 : 0);
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "cases")) {
    const double tf = 1.0 + 1e-6;  // synth.benchmark_radius: a radius just above a whole number of cells, tie-free
    auto base = [&](double rmax, double rmin, int rows, int cols, int batch = 1) {
      Case c;
      c.rmax_cells = rmax;
      c.rmin_cells = rmin;
      c.rows = rows;
      c.cols = cols;
      c.batch = batch;
      return c;
    };
    named("cfg3", base(9 * tf, 6 * tf, 4096, 4096));
    named("cfg3_any_reach_option", [&] { Case c = base(9 * tf, 6 * tf, 4096, 4096); c.opt_any = true; return c; }());
    named("reference_045_at_003", base(15.0, 10.0, 100, 133));  // 0.45 m at 0.03 m: a whole-cell tie radius of 15 cells
    named("reference_045_at_003_uploaded", [&] { Case c = base(15.0, 10.0, 100, 133); c.tcap = -1.0; return c; }());
    named("tie_free_9_uploaded", [&] { Case c = base(9 * tf, 6 * tf, 4096, 4096); c.tcap = -1.0; return c; }());
    named("tie_free_16", base(16 * tf, 10 * tf, 1024, 1024));
    named("reach_18", base(18.5, 12.0, 1024, 1024));
    named("reach_20_tie", base(20.0, 12.0, 1024, 1024));
    named("non_whole_tie_radius", base(std::sqrt(50.0), 4.0, 1024, 1024));  // 1-7 and 5-5: ties off the axis circle
    named("rows_48", base(9 * tf, 6 * tf, 48, 4096));
    named("cells_2_30", base(9 * tf, 6 * tf, 32768, 32768));
    named("reach_22_default_yaml_002", base(22.5, 15.0, 1024, 1024));
    named("reach_45_default_yaml_001", base(45.0, 30.0, 1024, 1024));
    named("rows_65", base(9 * tf, 6 * tf, 65, 4096));
    named("rows_4033", base(9 * tf, 6 * tf, 4033, 4033));
    named("rows_65_tie_15", base(15.0, 10.0, 65, 4096));
    named("rows_4033_tie_15", base(15.0, 10.0, 4033, 4033));
    named("cfg4_512_maps_of_512", base(9 * tf, 6 * tf, 512, 512, 512));
    named("cfg5_tile_256_of_8192", [&] {  // the 256 x 256 tile grown by the mask's 3 cells and the footprint's reach
      Case c = base(9 * tf, 6 * tf, 8192, 8192);
      c.region = true;
      c.i0 = c.j0 = 4096 - 12;
      c.i1 = c.j1 = 4096 + 256 + 12;
      return c;
    }());
    named("zero_rmin", base(9 * tf, 0.0, 4096, 4096));
    named("no_guard_rows", [&] { Case c = base(9 * tf, 6 * tf, 4096, 4096); c.guard_rows = false; return c; }());
    // ---- the cases of tests/test_gpu_footprint_values.py (tests/footprint_value_cases.py holds the same inputs) ----
    auto with = [&](Case c, double tcap, double def, bool opt_any = false) {
      c.tcap = tcap;
      c.def = def;
      c.opt_any = opt_any;
      return c;
    };
    // layers from outside (no bound): the inputs of k_fp_slide3 (tie-free 5 and 9) and of the general kernel (reach 18, a
    // whole-cell tie radius, a 48-row map), with the default 0.3, with fp_default = 50 and with TE_OPT_FP_ANY_REACH
    const struct { const char* name; double rmax, rmin; int rows, cols; } geos[] = {
        {"r5", 5 * tf, 3 * tf, 96, 80},     {"r9", 9 * tf, 6 * tf, 96, 80},     {"reach18", 18.5, 12.0, 96, 80},
        {"tie15", 15.0, 10.0, 96, 80},      {"rows48", 9 * tf, 6 * tf, 48, 80},
    };
    char name[96];
    for (const auto& q : geos) {
      snprintf(name, sizeof(name), "fv_ext_%s", q.name);
      named(name, with(base(q.rmax, q.rmin, q.rows, q.cols), -1.0, 0.3));
      snprintf(name, sizeof(name), "fv_ext_%s_def50", q.name);
      named(name, with(base(q.rmax, q.rmin, q.rows, q.cols), -1.0, 50.0));
      snprintf(name, sizeof(name), "fv_ext_%s_any", q.name);
      named(name, with(base(q.rmax, q.rmin, q.rows, q.cols), -1.0, 0.3, true));
    }
    // layers the chain wrote with plain weights: the sum of the scores (w_scale 1, weights 1 1 1) on a tie-free footprint
    // of 15 cells, weights 10 10 10 at 9 cells, a negative weight (no bound), a default of 50 under the default weights --
    // and the default weights at the same footprints, which keep their fixed-point kernels
    named("fv_w1111_r15", with(base(15 * tf, 10 * tf, 96, 80), 3.0, 0.3));
    named("fv_w1111_r15_batch2", with(base(15 * tf, 10 * tf, 96, 80, 2), 3.0, 0.3));
    named("fv_w1111_r15_region", [&] {  // te_run_chain_region(0, 21, 17, 31, 27): grown by 8 (the gap), 3 (the mask) and the reach
      Case c = with(base(15 * tf, 10 * tf, 96, 80), 3.0, 0.3);
      c.region = true;
      c.i0 = 0;
      c.i1 = 78;
      c.j0 = 0;
      c.j1 = 70;
      return c;
    }());
    named("fv_w1_10_r9", with(base(9 * tf, 6 * tf, 96, 80), 30.0, 0.3));
    named("fv_wneg_r9", with(base(9 * tf, 6 * tf, 96, 80), -1.0, 0.3));
    named("fv_def50_chain_r5", with(base(5 * tf, 3 * tf, 96, 80), (double)(1.0f / 3.0f) * 3.0, 50.0));
    named("fv_wdefault_r15", base(15 * tf, 10 * tf, 96, 80));
    named("fv_wdefault_r9", base(9 * tf, 6 * tf, 96, 80));
    // the boundary of the packed sums on a chain-written layer: the general kernel at reach 18 (1085 cells) with a bound
    // just below and just above 2048 / 1085
    named("fv_bound_below_reach18", with(base(18.5, 12.0, 96, 80), 1.88, 0.3));
    named("fv_bound_above_reach18", with(base(18.5, 12.0, 96, 80), 1.89, 0.3));
    // fixed point at saturation: w_scale (float) with weights 1 1 1 -- the largest that still gives k = 23 .. 17 and the first
    // that gives 16 -- for k_fp_slide5 at its largest disc (Q = 250, 793 cells) and k_fp_slide4 at the radii 15 and 16; the
    // default is the cap itself
    const struct { const char* name; double rmax, rmin; float s17, s16; } sats[] = {
        {"sat5", std::sqrt(250.0) * tf, 10 * tf, 0x1.b8c2a2p-2f, 0x1.b8c2a4p-2f},
        {"sat4_15", 15.0, 10.0, 0x1.6057d4p+0f, 0x1.6057d6p+0f},
        {"sat4_16", 16.0, 10.0, 0x1.4afd28p+0f, 0x1.4afd2ap+0f},
    };
    for (const auto& q : sats) {
      for (int k = 23; k >= 16; --k) {
        const float sc = k == 16 ? q.s16 : std::ldexp(q.s17, 17 - k);
        const double tcap = (double)sc * 3.0;
        snprintf(name, sizeof(name), "fv_%s_k%d", q.name, k);
        named(name, with(base(q.rmax, q.rmin, 96, 80), tcap, tcap));
      }
      // the cap is the default: small weights (a layer below 0.3), fp_default at the k = 17 cap
      snprintf(name, sizeof(name), "fv_%s_defcap", q.name);
      named(name, with(base(q.rmax, q.rmin, 96, 80), (double)0.1f * 3.0, (double)q.s17 * 3.0));
    }
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "sweep")) {
    const int n = atoi(argv[2]);
    std::mt19937 rng((unsigned)atoi(argv[3]));
    auto uni = [&](double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); };
    auto pick = [&](auto const& v) { return v[std::uniform_int_distribution<size_t>(0, sizeof(v) / sizeof(v[0]) - 1)(rng)]; };
    const int sizes[] = {1, 7, 33, 63, 64, 65, 100, 127, 128, 133, 257, 500, 1000, 1024, 4033, 4096, 8192, 16384, 32768};
    const int batches[] = {1, 1, 1, 2, 3, 8, 64, 512};
    const int cus[] = {32, 80, 104, 256, 304};
    const double tcaps[] = {-1.0, 0.0, 0.5, (double)(1.0f / 3.0f) * 3.0, 2.0, 100.0, 1e4};
    const double defs[] = {0.0, 0.3, 1.0, -0.5, 50.0};
    int failed = 0, by_route[5] = {0, 0, 0, 0, 0};
    for (int t = 0; t < n; ++t) {
      Case c;
      const double u = uni(0.0, 1.0);
      c.rmax_cells = u < 0.2 ? (double)(int)uni(1.0, 23.0) : u < 0.3 ? std::sqrt((double)(int)uni(2.0, 500.0)) : uni(0.5, 24.0);
      c.rmin_cells = uni(0.0, 1.0) < 0.15 ? 0.0 : uni(0.0, c.rmax_cells);
      c.rows = uni(0.0, 1.0) < 0.7 ? pick(sizes) : (int)uni(1.0, 9000.0);
      c.cols = uni(0.0, 1.0) < 0.7 ? pick(sizes) : (int)uni(1.0, 9000.0);
      c.batch = pick(batches);
      c.tcap = pick(tcaps);
      c.def = pick(defs);
      c.cus = pick(cus);
      c.opt_any = uni(0.0, 1.0) < 0.1;
      c.guard_rows = uni(0.0, 1.0) < 0.9;
      c.has_list = uni(0.0, 1.0) < 0.95;
      c.has_scratch = uni(0.0, 1.0) < 0.95;
      c.list_scale = uni(0.0, 1.0) < 0.85 ? 1.0 : uni(0.5, 1.0);
      if (uni(0.0, 1.0) < 0.3) {  // a region run: a non-empty rectangle of one map
        c.region = true;
        c.i0 = (int)uni(0.0, c.rows);
        c.i1 = c.i0 + 1 + (int)uni(0.0, c.rows - c.i0);
        c.j0 = (int)uni(0.0, c.cols);
        c.j1 = c.j0 + 1 + (int)uni(0.0, c.cols - c.j0);
        if (c.i1 > c.rows) c.i1 = c.rows;
        if (c.j1 > c.cols) c.j1 = c.cols;
      }
      const FpRouteIn in = inputs(c);
      const FpRoute r = plan_fp_route(in);
      by_route[r.route]++;
      char ctx[64];
      snprintf(ctx, sizeof(ctx), "sweep case %d", t);
      failed += check(in, r, ctx);
    }
    // every tie-free shape the fixed-point and the double kernel can take is instantiated: a route never lacks its kernel
    for (int a = 0; a <= 16; ++a)
      for (int b = a; b <= 16; ++b) {
        const int q = a * a + b * b;
        if (q < 1 || q > 256) continue;
        if (!fp_f3_shape(q) || (q < 256 && !fp_f5_shape(q))) {
          printf("FAIL shape %d is not instantiated\n", q);
          ++failed;
        }
      }
    printf("routes: slide5 %d, slide4 %d, slide3 %d, general %d, any %d\n", by_route[0], by_route[1], by_route[2], by_route[3], by_route[4]);
    printf("%d cases, %d failed checks\n", n, failed);
    return failed != 0;
  }
  if (argc >= 2 && !strcmp(argv[1], "constants")) {  // what tests/footprint_value_cases.py restates, from the header itself
    printf("kFpUOff %.17g\n", (double)kFpUOff);
    return 0;
  }
  fprintf(stderr, "usage: %s cases | sweep N SEED | constants\n", argv[0]);
  return 2;
}
