// raster_route_check.cpp -- the route plan of the filter chain (te_chain_route.h) under NormalVectorsFilter's raster method
// (ChainRouteIn::raster, TE_OPT_NORMALS_ALGORITHM = 1), and that nothing moved without it.  tests/test_raster_route.py.
//   raster_route_check raster N SEED   N seeded whole-map inputs (radii, sizes, batch, flags, hints) with `raster` set: never a
//                                      one-kernel route, always kNormalsRaster, the roughness stage the one
//                                      plan_filter_route(kFilterRoughness) gives, steps and combine as the text of the issue says;
//                                      TE_FILTER_NORMALS and region inputs too.  "N cases, F failed checks"
//   raster_route_check area N SEED     the same N inputs -- and region and per-plugin ones -- with `raster` false: one line per
//                                      input, "index hash" of every field of the plan (`full`: the fields themselves).
//                                      tests/golden/raster_route/area_plans.txt holds the lines the header of the commit before
//                                      the raster method printed (built with -DTE_ROUTE_CHECK_NO_RASTER, which leaves out the
//                                      fields that commit did not have).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

#include "te_chain_route.h"
#include "te_disc.h"
#include "te_hole_routing.h"

using namespace te;
using namespace te::fast;

static const double tf = 1.0 + 1e-6;  // a radius just above a whole number of cells: tie-free
static const double kRadii[] = {0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.0 * tf, 5.0 * tf, 5.0, 9.0 * tf, 9.0, 10.0, 12.0 * tf, 20.0 * tf, 33.0 * tf, 40.0};
static const int kSizes[][3] = {{3, 3, 1},   {2, 7, 1},     {1, 1, 1},     {67, 45, 1},     {65, 33, 2},     {128, 64, 1},   {131, 70, 3},
                                {100, 133, 1}, {512, 512, 1}, {1024, 512, 4}, {2048, 2048, 1}, {4096, 4096, 1}, {64, 4096, 1}, {40000, 30000, 1}};

static DiscSummary summary(double cells, double res, bool any) {
  Disc d;
  if (build_disc(cells * res, res, &d) != kDiscOk) any = true;
  if (any) {  // (the shim: a disc of te_filter_any.hip holds no runs)
    for (int b = 0; b <= kMaxRadiusCells; ++b) d.hw[b] = -1;
    d.Q = -1;
    d.any = 1;
  }
  return disc_summary(d);
}

struct Input {
  ChainRouteIn in;
  int filter = 0;  // 0: plan_chain_route; else plan_filter_route(filter)
};

template <class T, size_t N>
static const T& pick(std::mt19937& rng, const T (&a)[N]) {
  return a[rng() % N];
}

// One seeded input; `region` and `filter` inputs only where asked (the raster sweep plans whole maps and TE_FILTER_NORMALS)
static Input draw(std::mt19937& rng, bool allow_region_and_filters) {
  Input x;
  ChainRouteIn& in = x.in;
  const double res = (rng() % 4 == 0) ? 0.03 : 0.05;
  const bool any_all = rng() % 8 == 0;
  // one input in five is what the one-kernel routes take: a normals disc of one or two cells, its roughness disc the same, step
  // windows of a cell or 3 x 3
  static const double kSmallRadii[] = {1.0, 1.5, 2.0, 1.0, 2.0}, kSmallSteps[] = {0.5, 0.5, 1.0};
  const bool small_case = rng() % 5 == 0;
  const double rn = small_case ? pick(rng, kSmallRadii) : pick(rng, kRadii), rr = (small_case || rng() % 3 == 0) ? rn : pick(rng, kRadii);
  Disc dn, dr;
  const bool any_n = any_all || build_disc(rn * res, res, &dn) != kDiscOk, any_r = any_all || build_disc(rr * res, res, &dr) != kDiscOk;
  in.normals = summary(rn, res, any_all);
  in.rough = summary(rr, res, any_all);
  in.step1 = summary(small_case ? pick(rng, kSmallSteps) : pick(rng, kRadii), res, any_all);
  in.step2 = summary(small_case ? pick(rng, kSmallSteps) : pick(rng, kRadii), res, any_all);
  in.same_rough_disc = (any_n || any_r) ? (any_n && any_r && rn == rr) : same_disc(dn, dr);
  in.axis = rng() % 6 == 0 ? (int)(rng() % 2) : 2;
  in.res = res;
  const int* sz = pick(rng, kSizes);
  in.rows = sz[0];
  in.cols = sz[1];
  in.batch = sz[2];
  in.keep_normals = rng() % 2 == 0;
  in.normals_only = rng() % 6 == 0;
  in.generic_kernels = rng() % 6 == 0;
  const bool sequential = rng() % 4 == 0;
  in.defer_combine = !in.normals_only && !sequential && rng() % 3 == 0;
  const long long cells = (long long)in.rows * in.cols * in.batch;
  in.aux_stream = !sequential && cells >= (1ll << 21);
  static const double kHoles[] = {0.0, 0.0005, 0.01, 0.1, -1.0};
  const double hf = pick(rng, kHoles);
  HoleCounts h;
  h.cells = cells;
  h.invalid = hf < 0 ? -1 : (long long)(hf * (double)cells);
  h.runs = rng() % 2 ? h.invalid / 24 : h.invalid;
  in.sparse_holes = holes_sparse(h);
  in.hole_queue = in.sparse_holes;
  in.no_holes = h.invalid == 0;
  in.skip_clean = in.sparse_holes && holes_skip_clean_march(h);
  in.short_strips = holes_short_strips(h);
  in.clip_table = rng() % 16 != 0;
  in.tie_scratch = rng() % 16 != 0;
  in.block_flags = rng() % 16 != 0;
  in.guard_rows_elev = rng() % 16 != 0;
  in.guard_rows_step_height = rng() % 16 != 0;
  in.cus = rng() % 8 == 0 ? 64 : 256;
  const unsigned kind = rng() % 8;
  int a = (int)(rng() % (unsigned)in.rows), b = (int)(rng() % (unsigned)in.rows), c = (int)(rng() % (unsigned)in.cols), d = (int)(rng() % (unsigned)in.cols);
  if (allow_region_and_filters) {
    if (kind == 0) {
      in.whole = false;
      in.defer_combine = false;
      in.region = ChainRect{a < b ? a : b, c < d ? c : d, (a < b ? b : a) + 1, (c < d ? d : c) + 1};
    } else if (kind == 1)
      x.filter = kFilterStep;
    else if (kind == 2)
      x.filter = kFilterRoughness;
    else if (kind == 3)
      x.filter = kFilterNormals;
  } else if (kind == 3) {
    x.filter = kFilterNormals;
  }
  return x;
}

static ChainRoute plan(const Input& x) { return x.filter ? plan_filter_route(x.in, x.filter) : plan_chain_route(x.in); }

static std::string fields(const ChainRoute& r) {
  char buf[1024];
  int n = snprintf(buf, sizeof buf, "whole=%d sh=%d/%d ss=%d/%d normals=%d cross=%d keep=%d fixup=%d combine=%d two=%d steps=%d n3=%d/%d/%d/%d/%d", (int)r.whole,
                   (int)r.step_height.kind, r.step_height.Q, (int)r.step_score.kind, r.step_score.Q, (int)r.normals, (int)r.cross, (int)r.keep, (int)r.fixup,
                   (int)r.combine, (int)r.two_streams, (int)r.steps, r.n3_shape, r.n3_R, r.n3_resident, r.n3_blocks, (int)r.n3_short_strips);
  std::string s(buf, (size_t)n);
#define X(f) s += " " #f "=" + std::to_string(r.n3.f);
  TE_N3_STRIP_FIELDS(X)
#undef X
  const ChainRect* rc[4] = {&r.r_step1, &r.r_step2, &r.r_normals, &r.r_combine};
  for (const ChainRect* q : rc) s += " [" + std::to_string(q->i0) + "," + std::to_string(q->j0) + "," + std::to_string(q->i1) + "," + std::to_string(q->j1) + "]";
  return s;
}

static uint64_t fnv(const std::string& s) {
  uint64_t h = 1469598103934665603ull;
  for (unsigned char c : s) h = (h ^ c) * 1099511628211ull;
  return h;
}

static int run_area(int n, unsigned seed, bool full) {
  std::mt19937 rng(seed);
  for (int k = 0; k < n; ++k) {
    const Input x = draw(rng, true);
    const ChainRoute r = plan(x);
#ifndef TE_ROUTE_CHECK_NO_RASTER
    if (x.in.raster || r.raster_slope || r.rough != kNormalsNone || r.rough_fixup || r.normals == kNormalsRaster) {
      printf("FAIL case %d: an area plan carries a field of the raster method\n", k);
      return 1;
    }
#endif
    const std::string s = fields(r);
    if (full)
      printf("%d filter=%d whole=%d %dx%dx%d %s\n", k, x.filter, (int)x.in.whole, x.in.rows, x.in.cols, x.in.batch, s.c_str());
    else
      printf("%d %016llx\n", k, (unsigned long long)fnv(s));
  }
  return 0;
}

#ifndef TE_ROUTE_CHECK_NO_RASTER
static int run_raster(int n, unsigned seed) {
  std::mt19937 rng(seed);
  int bad = 0, n_rough[16] = {0}, n_filter = 0, n_only = 0, n_defer = 0, n_two = 0;
  auto req = [&](bool ok, int k, const char* what) {
    if (!ok) {
      ++bad;
      printf("FAIL case %d: %s\n", k, what);
    }
  };
  for (int k = 0; k < n; ++k) {
    Input x = draw(rng, false);
    const ChainRoute area = plan(x);
    x.in.raster = true;
    const ChainRoute r = plan(x);
    const bool only = x.in.normals_only || x.filter == kFilterNormals;
    req(r.whole == kWholeNone, k, "never a one-kernel route");
    req(r.normals == kNormalsRaster, k, "always kNormalsRaster");
    req(r.keep && !r.fixup && !r.cross, k, "the raster kernel writes the normal layers; no fix-up pass of its own");
    req(r.raster_slope == !only, k, "the slope is written unless the normals alone are asked for");
    // the roughness stage: what TE_FILTER_ROUGHNESS plans for the same inputs
    ChainRouteIn fin = x.in;
    fin.raster = false;
    const ChainRoute want = plan_filter_route(fin, kFilterRoughness);
    if (only) {
      req(r.rough == kNormalsNone && !r.rough_fixup && !r.steps && r.combine == kCombineNone && !r.two_streams, k, "normals only: nothing else runs");
    } else {
      req(r.rough == want.normals && r.rough_fixup == want.fixup, k, "roughness: the route plan_filter_route(kFilterRoughness) gives");
      req(r.rough == kNormalsAny || r.rough == kNormalsGeneric || r.rough == kNormalsSlideShape || r.rough == kNormalsSlideRadius, k,
          "roughness: sliding + fix-up, generic, or any radius");
      req(r.rough_fixup == (r.rough == kNormalsSlideShape || r.rough == kNormalsSlideRadius), k, "the fix-up pass follows the sliding kernel only");
      req(r.combine == (x.in.defer_combine ? kCombineDeferred : kCombineKernel), k, "the combine is k_combine or deferred");
      req(r.steps && r.two_streams == x.in.aux_stream, k, "the step filter runs, beside the normals when a second stream is handed in");
      // the step stages are planned as today: those of the area plan, unless that one fused them into one kernel
      const ChainRoute st = plan_filter_route(fin, kFilterStep);
      req(r.step_height.kind == st.step_height.kind && r.step_height.Q == st.step_height.Q && r.step_score.kind == st.step_score.kind &&
              r.step_score.Q == st.step_score.Q,
          k, "the step stages are those TE_FILTER_STEP plans");
      if (area.whole == kWholeNone)
        req(r.step_height.kind == area.step_height.kind && r.step_height.Q == area.step_height.Q && r.step_score.kind == area.step_score.kind &&
                r.step_score.Q == area.step_score.Q,
            k, "the step stages are the area plan's");
      ++n_rough[r.rough];
      n_defer += r.combine == kCombineDeferred;
      n_two += r.two_streams;
    }
    // the normals disc takes no part: another normals radius, the same plan
    Input y = x;
    y.in.normals = summary(y.in.normals.R == 7 ? 4.0 * tf : 7.0 * tf, y.in.res, false);
    y.in.same_rough_disc = !y.in.same_rough_disc;
    const ChainRoute r2 = plan(y);
    req(r2.normals == r.normals && r2.rough == r.rough && r2.rough_fixup == r.rough_fixup && r2.combine == r.combine && r2.steps == r.steps &&
            r2.step_height.kind == r.step_height.kind && r2.step_score.kind == r.step_score.kind && r2.two_streams == r.two_streams,
        k, "the normals radius plays no part in routing");
    // a region under raster is refused by the shim; the plan names no kernel for it
    ChainRouteIn rg = x.in;
    rg.whole = false;
    rg.region = ChainRect{0, 0, 1, 1};
    req(plan_chain_route(rg).normals == kNormalsNone, k, "a region under raster has no route");
    n_filter += x.filter == kFilterNormals;
    n_only += only;
  }
  printf("%d cases, %d failed checks\n", n, bad);
  printf("coverage: any=%d generic=%d slide_shape=%d slide_radius=%d normals_filter=%d normals_only=%d deferred=%d two_streams=%d\n", n_rough[kNormalsAny],
         n_rough[kNormalsGeneric], n_rough[kNormalsSlideShape], n_rough[kNormalsSlideRadius], n_filter, n_only, n_defer, n_two);
  return bad ? 1 : 0;
}
#endif

int main(int argc, char** argv) {
  if (argc >= 4 && !strcmp(argv[1], "area")) return run_area(atoi(argv[2]), (unsigned)atoi(argv[3]), argc >= 5 && !strcmp(argv[4], "full"));
#ifndef TE_ROUTE_CHECK_NO_RASTER
  if (argc >= 4 && !strcmp(argv[1], "raster")) return run_raster(atoi(argv[2]), (unsigned)atoi(argv[3]));
#endif
  fprintf(stderr, "usage: raster_route_check raster|area N SEED [full]\n");
  return 2;
}
