// chain_route_check.cpp -- the route of the filter chain from the header launch_chain / launch_filter route
// with (te_chain_route.h), on the discs of te_disc.h and the hole hints of te_hole_routing.h.  tests/test_chain_route.py.
//   chain_route_check cases         one line per named case: "name whole step_height step_score normals fixup combine streams"
//   chain_route_check sweep N SEED  N seeded cases; every route is held to what its kernels rely on: "N cases, F failed checks"
//   chain_route_check conditioning  reads "rows cols res radius-cells kept hole-fraction clustered generic any step1-cells
//                                   step2-cells batch" per line, prints the planned normals kernel in the words of
//                                   tests/test_gpu_conditioning.py's ids
//   chain_route_check filter        reads "rows cols batch res filter radius-cells second-radius-cells generic any hole-fraction
//                                   clustered" per line (filter: TE_FILTER_STEP, _ROUGHNESS or _NORMALS; the second radius is the step
//                                   filter's second window), prints plan_filter_route's route: the two step passes, or the normals kernel
//   chain_route_check params        reads "name rows cols batch res normals-cells roughness-cells step1-cells step2-cells axis kept generic
//                                   any footprint hole-fraction clustered region i0 j0 i1 j1 filter" per line (any: the value of
//                                   TE_OPT_FILTER_ANY_RADIUS; footprint: the mask kernel combines; region: 0 a whole-map run, 1 the
//                                   half-open rectangle that follows; filter: 0 the chain, else TE_FILTER_*), prints the plan as `cases` does
#include <cmath>
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

struct Case {
  double rn = 9, rr = 9, s1 = 9, s2 = 9;  // radii in cells: normals, roughness, the two step windows
  double res = 0.05;
  int rows = 4096, cols = 4096, batch = 1;
  bool region = false;
  ChainRect rect = {0, 0, 0, 0};
  bool keep = false, normals_only = false, generic = false, defer = false, sequential = false;
  double hole_fraction = 0.0;  // of the cells, counted at upload; < 0: unknown
  bool clustered = false;      // ... in runs of 24 cells
  bool any[4] = {false, false, false, false};  // TE_OPT_FILTER_ANY_RADIUS: normals, roughness, step 1, step 2
  int axis = 2;
  bool guard_elev = true, guard_sh = true, clip = true, scratch = true, flags = true;
  int cus = 256;
  int filter = 0;  // 0: launch_chain; else TE_FILTER_* through plan_filter_route
};

static const double tf = 1.0 + 1e-6;  // synth.benchmark_radius: a radius just above a whole number of cells, tie-free

static DiscSummary summary(double cells, double res, bool any, Disc* out) {
  Disc d;
  if (build_disc(cells * res, res, &d) != kDiscOk) any = true;
  if (any) {  // (the shim: a disc of te_filter_any.hip holds no runs)
    for (int b = 0; b <= kMaxRadiusCells; ++b) d.hw[b] = -1;
    d.Q = -1;
    d.any = 1;
  }
  if (out) *out = d;
  return disc_summary(d);
}

// the plan's inputs as launch_chain fills them; the hints as the shim derives them from the upload's counts
static ChainRouteIn inputs(const Case& c) {
  ChainRouteIn in;
  Disc dn, dr;
  in.normals = summary(c.rn, c.res, c.any[0], &dn);
  in.rough = summary(c.rr, c.res, c.any[1], &dr);
  in.step1 = summary(c.s1, c.res, c.any[2], nullptr);
  in.step2 = summary(c.s2, c.res, c.any[3], nullptr);
  in.same_rough_disc = (dn.any || dr.any) ? (dn.any && dr.any && c.rn == c.rr) : same_disc(dn, dr);
  in.axis = c.axis;
  in.res = c.res;
  in.rows = c.rows;
  in.cols = c.cols;
  in.batch = c.batch;
  in.whole = !c.region;
  in.region = c.rect;
  in.keep_normals = c.keep;
  in.normals_only = c.normals_only;
  in.generic_kernels = c.generic;
  in.defer_combine = c.defer && !c.region;  // (only a whole-map launch with the footprint pass behind it defers)
  const long long cells = (long long)c.rows * c.cols * c.batch;
  in.aux_stream = !c.sequential && cells >= (1ll << 21);
  HoleCounts h;
  h.cells = cells;
  h.invalid = c.hole_fraction < 0 ? -1 : (long long)std::llround(c.hole_fraction * (double)cells);
  h.runs = c.clustered ? h.invalid / 24 : h.invalid;
  in.sparse_holes = holes_sparse(h);
  in.hole_queue = in.sparse_holes;  // (allocated on first need)
  in.no_holes = h.invalid == 0;
  in.skip_clean = in.sparse_holes && holes_skip_clean_march(h);
  in.short_strips = holes_short_strips(h);
  in.clip_table = c.clip;
  in.tie_scratch = c.scratch;
  in.block_flags = c.flags;
  in.guard_rows_elev = c.guard_elev;
  in.guard_rows_step_height = c.guard_sh;
  in.cus = c.cus;
  return in;
}

static ChainRoute plan(const ChainRouteIn& in, const Case& c) { return c.filter ? plan_filter_route(in, c.filter) : plan_chain_route(in); }

static const char* kWhole[] = {"none", "k_chain_window", "k_normals_small+step+combine"};
static const char* kCombine[] = {"none", "in_normals", "k_combine", "deferred", "in_chain"};
static const char* kNormals[] = {"k_normals_small", "k_normals3s", "k_normals3-sparse", "k_normals3-dense", "k_normals3-TIES", "k_normals_slide",
                                 "k_normals_slide<R>", "k_normals", "any", "-"};

static std::string step_name(const StepRoute& s, bool ran) {
  if (!ran) return "-";
  switch (s.kind) {
    case kStepSmall: return "k_step_small";
    case kStepMarch: return "march<" + std::to_string(s.Q) + ">";
    case kStepMarchTies: return "RAW<" + std::to_string(s.Q) + ">+ties";
    case kStepGeneric: return "generic";
    default: return "any";
  }
}
static std::string normals_name(const ChainRoute& r) {
  std::string s = kNormals[r.normals];
  if (r.normals == kNormalsSmall && r.cross) s += "-CROSS";
  if (r.keep && (r.normals == kNormals3Dense || r.normals == kNormals3Ties)) s.insert(s.find('-') + 1, "KEEP-");
  if (r.normals == kNormals3Dense && r.n3_short_strips) s += "-short";
  return s;
}

// what the kernels of the route rely on -- today's early returns, each stated once; returns the number of failed checks
static int check(const ChainRouteIn& in, const ChainRoute& r, const Case& c, const char* ctx) {
  int bad = 0;
  auto req = [&](bool ok, const char* what) {
    if (!ok) {
      ++bad;
      printf("FAIL %s: %s (%d x %d x %d, normals R %d Q %d reach %d ties %d)\n", ctx, what, in.rows, in.cols, in.batch, in.normals.R, in.normals.Q,
             in.normals.reach, in.normals.n_ties);
    }
  };
  const DiscSummary& d = c.filter == kFilterRoughness ? in.rough : in.normals;
  const double map_bytes = (double)in.rows * in.cols * 4.0;
  const int maps = in.whole ? in.batch : 1;
  const bool n3 = r.normals == kNormals3Slim || r.normals == kNormals3Sparse || r.normals == kNormals3Dense || r.normals == kNormals3Ties;
  const bool small = r.normals == kNormalsSmall || r.whole == kWholeNormalsSmall;
  const int wn = r.r_normals.i1 - r.r_normals.i0;
  if (n3) {
    const int R = r.n3_R;
    req(n3_shape(r.n3_shape) && isqrt_c(r.n3_shape) == R, "k_normals3: the shape is instantiated (TE_N3_P*)");
    req(wn >= 64 && in.rows >= 2 * R + 1 && in.cols >= 2 * R + 1 && map_bytes < 4294967296.0, "k_normals3: 64 wide, a map that holds the disc, under 4 GiB");
    req(in.clip_table, "k_normals3: the clip table");
    req(in.res * in.res * (double)(d.sii_runs + d.sii_ties) / (double)(d.npoints + d.n_ties) > 1e-8, "k_normals3: the conditioning test");
    req(r.fixup, "k_normals3: the fix-up pass follows");
    req(r.n3_blocks > 0 && r.n3.rows_int >= 1, "k_normals3: a strip plan");
    req(d.n_ties == 0 ? r.n3_shape == d.Q : r.normals == kNormals3Ties, "k_normals3: tie radii take the TIES march");
  }
  if (r.normals == kNormals3Sparse)
    req(in.hole_queue && in.sparse_holes && !r.keep && (long long)r.n3_blocks * maps <= 12ll * in.cus, "sparse: a queue for every block");
  if (r.normals == kNormals3Slim)
    req(n3_slim_shape(r.n3_shape) && in.no_holes && !r.keep && d.n_ties == 0, "slim: slim shape, no holes, not kept, no ties");
  if (r.normals == kNormals3Ties)
    req(r.n3_R >= 3 && r.n3_shape == r.n3_R * r.n3_R && d.ties_on_circle && d.n_gen == tie_triple_cells(r.n3_R) && d.n_ties == 4 + d.n_gen,
        "TIES: the circle's cells are the ones the kernel knows");
  if (small) {
    req(d.reach >= 1 && d.reach <= 2 && d.n_offsets >= 2 && d.n_offsets <= kSmallOffsets && map_bytes < 4294967296.0, "k_normals_small: reach 1..2, 2..12 offsets");
    req(!r.fixup, "k_normals_small settles every cell itself");
    req(!r.cross || (d.n_ties == 4 && d.npoints == 1), "CROSS: the four edge neighbours, all on the circle");
  }
  if (r.whole == kWholeChainWindow)
    req(in.whole && (long long)in.rows * in.cols * in.batch <= (1ll << 18) && in.step1.Q >= 0 && in.step1.Q <= 2 && in.step2.Q >= 0 && in.step2.Q <= 2 &&
            in.step1.n_ties == 0 && in.step2.n_ties == 0 && d.reach >= 1 && d.reach <= 2 && d.npoints + d.n_ties >= 3,
        "k_chain_window: <= 2^18 cells, step windows within 3 x 3 and tie-free, a disc within two cells, whole map");
  if (r.whole != kWholeNone)
    req(in.whole && !in.generic_kernels && !in.normals_only && in.same_rough_disc && in.axis == 2 && !in.normals.any && !in.rough.any && !in.step1.any &&
            !in.step2.any && !r.two_streams && (r.combine == kCombineInChain || r.combine == kCombineDeferred),
        "a one-kernel chain: whole maps, the fast kernels' parameters, no disc of any radius");
  if (r.whole == kWholeNormalsSmall) req(in.step1.Q == 0 && in.step2.Q == 0, "k_normals_small writes the step layer only for single-cell windows");
  if (r.normals == kNormalsSlideShape || r.normals == kNormalsSlideRadius) {
    req(d.n_ties == 0 && slide_radius(d.R) && d.npoints >= 3 && in.rows >= 2 * d.R + 1 && in.cols >= 2 * d.R + 1 && r.fixup, "k_normals_slide: tie-free, R 1..16");
    req(r.normals == kNormalsSlideRadius || (d.Q >= 1 && disc_shape(d.Q)), "k_normals_slide: the shape is instantiated");
    req(c.filter == kFilterRoughness ? in.block_flags : in.clip_table, "k_normals_slide: its table / flags");
  }
  if (c.filter == 0 && r.normals != kNormalsGeneric && r.normals != kNormalsAny && r.whole == kWholeNone)
    req(!in.generic_kernels && in.same_rough_disc && in.axis == 2, "a shape-specialised normals kernel: same disc, axis z");
  if (c.filter == 0 && r.whole == kWholeNone) req((r.normals == kNormalsAny) == ((in.normals.any || in.rough.any)), "a disc marked any takes the route of any radius for its stage");
  // normal_vector_positive_axis x or y: only the kernels that read the axis
  if (in.axis != 2 && (c.filter == 0 || c.filter == kFilterNormals))
    req(r.whole == kWholeNone && (r.normals == kNormalsGeneric || r.normals == kNormalsAny || r.normals == kNormalsRaster) && !r.fixup,
        "axis x / y: no one-kernel chain, and k_normals, the route of any radius or raster");
  const StepRoute* st[2] = {&r.step_height, &r.step_score};
  const DiscSummary* sd[2] = {&in.step1, &in.step2};
  const ChainRect* sr[2] = {&r.r_step1, &r.r_step2};
  const bool guard[2] = {in.guard_rows_elev, in.guard_rows_step_height};
  const bool steps = (c.filter == 0 && r.whole == kWholeNone && !in.normals_only) || c.filter == kFilterStep;
  for (int k = 0; k < 2 && steps; ++k) {
    const StepRoute& s = *st[k];
    req((s.kind == kStepAny) == sd[k]->any, "a step disc marked any takes the route of any radius");
    if (s.kind == kStepMarch || s.kind == kStepMarchTies)
      req(sr[k]->i1 - sr[k]->i0 >= 64 && guard[k] && disc_shape(s.Q) && !in.generic_kernels, "march: 64 wide, guard rows, shape instantiated");
    if (s.kind == kStepMarch) req(sd[k]->n_ties == 0 && s.Q == sd[k]->Q, "march: the tie-free disc's own shape");
    if (s.kind == kStepMarchTies) req(step_raw_shape(s.Q) && in.tie_scratch && sd[k]->ties_on_circle && s.Q == sd[k]->q_runs, "RAW: a RAW shape, the scratch");
    if (s.kind == kStepSmall) req(sd[k]->n_ties == 0 ? sd[k]->Q == 0 : (sd[k]->reach <= 2 && sd[k]->n_offsets <= kSmallOffsets), "k_step_small: its window");
  }
  // the combine happens exactly once, or is deferred, or is absent under normals only
  if (c.filter == 0) {
    req((r.combine == kCombineNone) == in.normals_only, "no combine exactly under normals only");
    req((r.combine == kCombineDeferred) == (in.defer_combine && !in.normals_only), "deferred exactly when the mask kernel combines");
    req(r.combine != kCombineInChain || r.whole != kWholeNone, "in the one-kernel chain only there");
    req(r.combine != kCombineInNormals || (in.whole && !r.two_streams && !small && !n3), "fused only behind a complete step layer, in a kernel that can");
    req(r.two_streams == (in.whole && in.aux_stream && !in.normals_only && r.whole == kWholeNone), "two streams only on whole runs");
  }
  return bad;
}

static int named(const char* name, const Case& c) {
  const ChainRouteIn in = inputs(c);
  const ChainRoute r = plan(in, c);
  if (check(in, r, c, name)) exit(1);
  const bool steps = (c.filter == 0 && r.whole == kWholeNone && !in.normals_only) || c.filter == kFilterStep;
  printf("%s %s %s %s %s %d %s %d\n", name, kWhole[r.whole], step_name(r.step_height, steps).c_str(), step_name(r.step_score, steps).c_str(),
         r.whole != kWholeNone ? "-" : normals_name(r).c_str(), r.fixup ? 1 : 0, kCombine[r.combine], r.two_streams ? 1 : 0);
  return 0;
}

static Case radius(double cells, int rows, int cols, int batch = 1) {
  Case c;
  c.rn = c.rr = c.s1 = c.s2 = cells;
  c.rows = rows;
  c.cols = cols;
  c.batch = batch;
  return c;
}
static Case defaults(double res, int rows, int cols) {  // robot_filter_parameter.yaml: normals / roughness 0.05 m, step windows 0.04 m
  Case c = radius(0.05 / res, rows, cols);
  c.s1 = c.s2 = 0.04 / res;
  c.res = res;
  return c;
}
template <class F>
static Case with(Case c, F f) {
  f(c);
  return c;
}

static void all_cases() {
  const Case cfg3 = radius(9 * tf, 4096, 4096);
  named("cfg3", cfg3);
  named("cfg3_footprint", with(cfg3, [](Case& c) { c.defer = true; }));
  named("cfg3_speckle_0.1%", with(cfg3, [](Case& c) { c.hole_fraction = 0.001; }));
  named("cfg3_speckle_5%", with(cfg3, [](Case& c) { c.hole_fraction = 0.05; }));
  named("cfg3_regions", with(cfg3, [](Case& c) { c.hole_fraction = 0.05; c.clustered = true; }));
  named("cfg3_kept", with(cfg3, [](Case& c) { c.keep = true; }));
  named("cfg3_sequential", with(cfg3, [](Case& c) { c.sequential = true; }));
  named("cfg4_512_maps_of_512_speckle", with(radius(5 * tf, 512, 512, 512), [](Case& c) { c.hole_fraction = 0.001; }));
  named("tie_3", radius(3, 4096, 4096));
  named("tie_4", radius(4, 4096, 4096));
  named("tie_10", radius(10, 4096, 4096));
  named("default_yaml_005_4096", defaults(0.05, 4096, 4096));
  named("default_yaml_005_1024", defaults(0.05, 1024, 1024));
  named("bag_map_100x133_003", defaults(0.03, 100, 133));
  named("default_yaml_005_2^18", defaults(0.05, 512, 512));
  named("default_yaml_005_2^18+64", defaults(0.05, 64, 4097));
  named("tie_free_reach2_2^18+64", with(radius(1.5, 64, 4097), [](Case& c) { c.s1 = c.s2 = 0.8; }));
  named("rows_48", radius(5 * tf, 48, 4096));
  named("rows_64", radius(5 * tf, 64, 4096));
  named("radius_11", radius(11 * tf, 1024, 1024));
  named("radius_16", radius(16 * tf, 1024, 1024));
  named("radius_17", radius(17 * tf, 1024, 1024));
  named("normals_5_roughness_7", with(radius(5 * tf, 1024, 1024), [](Case& c) { c.rr = 7 * tf; }));
  named("axis_x", with(radius(5 * tf, 1024, 1024), [](Case& c) { c.axis = 0; }));
  named("generic_kernels", with(cfg3, [](Case& c) { c.generic = true; }));
  const char* any_names[4] = {"any_normals", "any_roughness", "any_step1", "any_step2"};
  for (int k = 0; k < 4; ++k) named(any_names[k], with(radius(5 * tf, 1024, 1024), [k](Case& c) { c.any[k] = true; }));
  named("cells_2^30", radius(9 * tf, 32768, 32768));
  named("narrower_than_the_disc", radius(9 * tf, 4096, 17));
  named("step_one_cell", with(radius(5 * tf, 1024, 1024), [](Case& c) { c.s1 = c.s2 = 0.8; }));
  named("step_tie_1", with(radius(5 * tf, 1024, 1024), [](Case& c) { c.s1 = c.s2 = 1; }));
  named("step_tie_2", with(radius(5 * tf, 1024, 1024), [](Case& c) { c.s1 = c.s2 = 2; }));
  named("step_5", radius(5 * tf, 1024, 1024));
  named("step_no_guard_rows", with(radius(5 * tf, 1024, 1024), [](Case& c) { c.guard_elev = c.guard_sh = false; }));
  named("step_region_narrower_than_64", with(radius(5 * tf, 1024, 1024), [](Case& c) { c.region = true; c.rect = ChainRect{500, 500, 520, 600}; }));
  named("cfg5_tile_256_of_8192", with(radius(5 * tf, 8192, 8192), [](Case& c) { c.region = true; c.rect = ChainRect{4096, 4096, 4352, 4352}; }));
  named("normals_only", with(cfg3, [](Case& c) { c.normals_only = true; }));
  // launch_filter: each TE_FILTER_*
  const char* fnames[6] = {"", "filter_slope", "filter_step", "filter_roughness", "filter_combine", "filter_normals"};
  for (int f = 1; f <= 5; ++f) named(fnames[f], with(radius(5 * tf, 1024, 1024), [f](Case& c) { c.filter = f; }));
  named("filter_roughness_tie", with(radius(4, 1024, 1024), [](Case& c) { c.filter = kFilterRoughness; }));
  named("filter_roughness_any", with(radius(5 * tf, 1024, 1024), [](Case& c) { c.filter = kFilterRoughness; c.any[1] = true; }));
  named("filter_roughness_16", with(radius(16 * tf, 1024, 1024), [](Case& c) { c.filter = kFilterRoughness; }));
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "cases")) {
    all_cases();
    const Case c = with(radius(5 * tf, 8192, 8192), [](Case& c) { c.region = true; c.rect = ChainRect{4096, 4096, 4352, 4352}; });
    const ChainRoute r = plan_chain_route(inputs(c));  // k_combine on the region grown by the chain's reach (both step windows: 10)
    printf("cfg5_combine_rect %d %d %d %d\n", r.r_combine.i0, r.r_combine.j0, r.r_combine.i1, r.r_combine.j1);
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "sweep")) {
    const int n = atoi(argv[2]);
    std::mt19937 rng((unsigned)atoi(argv[3]));
    auto uni = [&](double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); };
    auto pick = [&](auto const& v) { return v[std::uniform_int_distribution<size_t>(0, sizeof(v) / sizeof(v[0]) - 1)(rng)]; };
    auto coin = [&](double p) { return uni(0.0, 1.0) < p; };
    const int sizes[] = {1, 7, 17, 33, 48, 63, 64, 65, 100, 128, 133, 257, 512, 1000, 1024, 2048, 4033, 4096, 8192, 32768};
    const int batches[] = {1, 1, 1, 2, 3, 64, 512};
    const int cus[] = {32, 104, 256, 304};
    const double fractions[] = {0.0, 0.0, 0.0005, 0.001, 0.002, 0.01, 0.05, -1.0};
    const double ress[] = {0.05, 0.05, 0.03, 0.5, 1e-5};
    int failed = 0, whole[3] = {}, step[5] = {}, normals[10] = {}, combine[5] = {}, flags[6] = {};
    auto radius_of = [&]() {
      const double u = uni(0.0, 1.0);
      return u < 0.3 ? (double)(int)uni(0.0, 12.0) : u < 0.4 ? std::sqrt((double)(int)uni(1.0, 300.0)) : u < 0.8 ? uni(0.3, 11.0) : uni(0.3, 20.0);
    };
    for (int t = 0; t < n; ++t) {
      Case c;
      c.rn = radius_of();
      c.rr = coin(0.8) ? c.rn : radius_of();
      c.s1 = radius_of();
      c.s2 = coin(0.7) ? c.s1 : radius_of();
      c.res = pick(ress);
      c.rows = coin(0.7) ? pick(sizes) : (int)uni(1.0, 5000.0);
      c.cols = coin(0.7) ? pick(sizes) : (int)uni(1.0, 5000.0);
      c.batch = pick(batches);
      if ((double)c.rows * c.cols * c.batch > 4e9) c.batch = 1;
      c.keep = coin(0.3);
      c.normals_only = coin(0.05);
      c.generic = coin(0.05);
      c.defer = coin(0.3);
      c.sequential = coin(0.2);
      c.hole_fraction = pick(fractions);
      c.clustered = coin(0.3);
      for (bool& a : c.any) a = coin(0.04);
      c.axis = coin(0.95) ? 2 : 0;
      c.guard_elev = coin(0.95);
      c.guard_sh = coin(0.95);
      c.clip = coin(0.97);
      c.scratch = coin(0.95);
      c.flags = coin(0.97);
      c.cus = pick(cus);
      c.filter = coin(0.85) ? 0 : 1 + (int)uni(0.0, 5.0);
      if (c.filter == 0 && coin(0.25)) {  // a region run: a non-empty rectangle of one map
        c.region = true;
        c.rect.i0 = (int)uni(0.0, c.rows);
        c.rect.i1 = std::min(c.rows, c.rect.i0 + 1 + (int)uni(0.0, 300.0));
        c.rect.j0 = (int)uni(0.0, c.cols);
        c.rect.j1 = std::min(c.cols, c.rect.j0 + 1 + (int)uni(0.0, 300.0));
      }
      const double kind = uni(0.0, 1.0);
      if (kind < 0.15) {  // the reference's defaults and their neighbours: discs within two cells, step windows within 3 x 3
        const double small_r[] = {1.0, 1.2, 1.5, 2.0}, small_s[] = {0.8, 0.8, 1.2, 1.0};
        c.rn = c.rr = pick(small_r);
        c.s1 = c.s2 = pick(small_s);
        c.res = 0.05;
        c.filter = 0;
        c.region = c.generic = c.normals_only = false;
        c.axis = 2;
        for (bool& a : c.any) a = false;
        if (coin(0.5)) c.rows = 128, c.cols = 100, c.batch = 1;
      } else if (kind < 0.25) {  // the benchmark's: tie-free 9 and 10 cells on a hole-free map
        c.rn = c.rr = coin(0.5) ? 9 * tf : 10 * tf;
        c.res = 0.05;
        c.hole_fraction = 0.0;
        c.rows = std::max(c.rows, 64);
        c.cols = std::max(c.cols, 64);
        c.axis = 2;
      }
      const ChainRouteIn in = inputs(c);
      const ChainRoute r = plan(in, c);
      char ctx[64];
      snprintf(ctx, sizeof(ctx), "sweep case %d", t);
      failed += check(in, r, c, ctx);
      whole[r.whole]++;
      if (r.whole == kWholeNone && (c.filter == 0 || c.filter == kFilterStep)) step[r.step_height.kind]++, step[r.step_score.kind]++;
      normals[r.normals]++;
      combine[r.combine]++;
      flags[0] += r.cross, flags[1] += r.keep, flags[2] += r.fixup, flags[3] += r.two_streams, flags[4] += r.n3_short_strips, flags[5] += !r.keep;
    }
    // every shape a tie-free disc up to 10 cells can take is instantiated where the plan sends it, every RAW shape is a disc shape
    for (int a = 0; a <= 10; ++a)
      for (int b = a; b <= 10; ++b) {
        const int q = a * a + b * b;
        if (q <= 100 && (!disc_shape(q) || (q >= 1 && !n3_shape(q)))) printf("FAIL shape %d is not instantiated\n", q), ++failed;
      }
    for (int R = 3; R <= 10; ++R) {
      Disc d;
      build_disc(R * 0.05, 0.05, &d);
      if (!step_raw_shape(disc_summary(d).q_runs) || !disc_shape(disc_summary(d).q_runs)) printf("FAIL RAW shape of radius %d\n", R), ++failed;
    }
    auto row = [](const char* what, const int* v, int k) {
      printf("%s:", what);
      for (int i = 0; i < k; ++i) printf(" %d", v[i]);
      printf("\n");
    };
    row("whole", whole, 3);
    row("step", step, 5);
    row("normals", normals, 10);
    row("combine", combine, 5);
    row("flags", flags, 6);
    printf("%d cases, %d failed checks\n", n, failed);
    return failed != 0;
  }
  if (argc >= 2 && !strcmp(argv[1], "conditioning")) {
    Case c;
    double cells;
    int kept, clustered, generic, any;
    while (scanf("%d %d %lf %lf %d %lf %d %d %d %lf %lf %d", &c.rows, &c.cols, &c.res, &cells, &kept, &c.hole_fraction, &clustered, &generic, &any, &c.s1,
                 &c.s2, &c.batch) == 12) {
      c.rn = c.rr = cells;
      c.keep = kept != 0;
      c.clustered = clustered != 0;
      c.generic = generic != 0;
      for (bool& a : c.any) a = any != 0;
      const ChainRouteIn in = inputs(c);
      const ChainRoute r = plan_chain_route(in);
      if (check(in, r, c, "conditioning")) return 1;
      // the words of the ids: the TE_RUN_GENERIC_KERNELS route is named with the fix-up pass of its family, the route of any radius by
      // its two kernels, the dense march on a hole-free map "clean"
      std::string s = r.whole == kWholeChainWindow ? "k_chain_window" : r.whole == kWholeNormalsSmall ? "k_normals_small" : normals_name(r);
      if (r.whole == kWholeNone && r.normals == kNormalsGeneric && in.generic_kernels) s = "k_normals+k_normals_fixup";
      if (r.whole == kWholeNone && r.normals == kNormalsAny) s = "k_fa_normals+k_fa_exact";
      if (r.normals == kNormalsSmall && r.whole == kWholeNone) s = "k_normals_small";
      if (r.normals == kNormals3Dense && !r.keep) s = in.no_holes ? "k_normals3-clean" : "k_normals3-dense";
      if (r.normals == kNormals3Dense && r.keep) s = "k_normals3-KEEP-dense";
      if (r.normals == kNormals3Ties) s = "k_normals3-TIES";
      printf("%s\n", s.c_str());
    }
    return 0;
  }
  if (argc >= 2 && !strcmp(argv[1], "filter")) {
    Case c;
    double r1, r2;
    int generic, any, clustered;
    while (scanf("%d %d %d %lf %d %lf %lf %d %d %lf %d", &c.rows, &c.cols, &c.batch, &c.res, &c.filter, &r1, &r2, &generic, &any, &c.hole_fraction,
                 &clustered) == 11) {
      if (c.filter != kFilterStep && c.filter != kFilterRoughness && c.filter != kFilterNormals) return 1;
      // (the discs of the other filters: the parameters' defaults, which no single plugin's plan reads)
      c.rn = c.rr = c.s1 = c.s2 = 0.05 / c.res;
      if (c.filter == kFilterStep) c.s1 = r1, c.s2 = r2;
      if (c.filter == kFilterRoughness) c.rr = r1;
      if (c.filter == kFilterNormals) c.rn = r1;
      c.generic = generic != 0;
      c.clustered = clustered != 0;
      for (bool& a : c.any) a = any != 0;
      const ChainRouteIn in = inputs(c);
      const ChainRoute r = plan(in, c);
      if (check(in, r, c, "filter")) return 1;
      if (c.filter == kFilterStep)
        printf("%s %s\n", step_name(r.step_height, true).c_str(), step_name(r.step_score, true).c_str());
      else
        printf("%s\n", normals_name(r).c_str());
    }
    return 0;
  }
  if (argc >= 2 && !strcmp(argv[1], "params")) {
    char name[128];
    Case c;
    int kept, generic, any, footprint, clustered, region;
    while (scanf("%127s %d %d %d %lf %lf %lf %lf %lf %d %d %d %d %d %lf %d %d %d %d %d %d %d", name, &c.rows, &c.cols, &c.batch, &c.res, &c.rn, &c.rr, &c.s1, &c.s2,
                 &c.axis, &kept, &generic, &any, &footprint, &c.hole_fraction, &clustered, &region, &c.rect.i0, &c.rect.j0, &c.rect.i1, &c.rect.j1,
                 &c.filter) == 22) {
      if (c.axis < 0 || c.axis > 2 || c.filter < 0 || c.filter > kFilterNormals) return 1;
      if (region && !(c.rect.i0 >= 0 && c.rect.j0 >= 0 && c.rect.i0 < c.rect.i1 && c.rect.j0 < c.rect.j1 && c.rect.i1 <= c.rows && c.rect.j1 <= c.cols)) return 1;
      c.keep = kept != 0;
      c.generic = generic != 0;
      c.defer = footprint != 0;
      c.clustered = clustered != 0;
      c.region = region != 0;
      for (bool& a : c.any) a = any == 2;  // (option 1: only the discs build_disc refuses, which summary() marks)
      named(name, c);
    }
    return 0;
  }
  fprintf(stderr, "usage: %s cases | sweep N SEED | conditioning < lines | filter < lines | params < lines\n", argv[0]);
  return 2;
}
