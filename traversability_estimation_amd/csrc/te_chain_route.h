// te_chain_route.h -- which kernels run the filter chain (normals, slope and roughness; both step passes; the combine):
// DESIGN.md 4.7, decided once per launch on the host.  Plain C++ of plain values: launch_chain and launch_filter
// (te_kernels.hip) fill ChainRouteIn, call the plan and switch on its fields; the launchers of the routes decide nothing,
// and a planned route whose shape is not instantiated is an error, never a slower kernel.  The CPU check
// (tests/cpu/chain_route_check.cpp, tests/test_chain_route.py) runs the same code on DESIGN.md's cases and on a sweep, and
// holds every route to what its kernels rely on.
#pragma once
#include "te_disc.h"
#include "te_n3_plan.h"
#include "te_shapes.h"
#include "te_tie_triple.h"

namespace te {
namespace fast {

constexpr int kSmallOffsets = 12;     // k_normals_small, k_step_small: offsets besides the centre (the 13-point disc: reach 2)
constexpr long long kSmallLaunchCells = 1ll << 18;  // tie-free discs take k_normals_small up to here; k_chain_window's limit
constexpr int kN3RouteWaves = 3;           // waves per SIMD k_normals3 / k_normals3s are compiled for
constexpr int kN3RouteTieWaves = 3;        // ... and the TIES march

// LDS of one single-wave block of k_normals3 (the ring of 2R+2 rows and the hole masks) and of k_normals3s (the slim ring
// of 2R rows); te_normals3.hip asserts its declarations against these
constexpr int n3_lds_bytes(int R, bool slim) {
  return slim ? (2 * R) * (kN3Lanes + 2 * R) * 8 : (2 * R + 2) * (kN3Lanes + 2 * R) * 8 + (2 * R + 2) * 16;
}
// single-wave blocks the LDS admits per CU (2 KiB granules, tools/census.hip: at R = 9, 13 120 B, 11 fit and not 12), at most
// `waves` per SIMD
constexpr int n3_blocks_per_cu(int lds_bytes, int waves = kN3RouteWaves) {
  const int n = (160 * 1024) / (((lds_bytes + 2047) / 2048) * 2048);
  return n > waves * 4 ? waves * 4 : n;
}
// The slim ring only where the centre column alone reaches rows j +- R and the two rows saved buy a resident block: R = 9
// (11 -> 12 per CU) and R = 10 (10 -> 11); at smaller radii the slim march measured 2 % slower
constexpr bool n3_slim_shape(int q) {
  const int R = isqrt_c(q);
  return q >= 1 && R >= 2 && isqrt_c(q - 1) < R && n3_blocks_per_cu(n3_lds_bytes(R, true)) > n3_blocks_per_cu(n3_lds_bytes(R, false));
}
// resident blocks per CU of a launch (override: TE_N3_BLOCKS_PER_CU; the hole queues are allocated for kN3RouteWaves * 4 per CU)
constexpr int n3_resident_per_cu(int R, bool slim, bool ties, int override_per_cu) {
  int per_cu = n3_blocks_per_cu(n3_lds_bytes(R, slim));
  if (!slim && ties && per_cu > kN3RouteTieWaves * 4) per_cu = kN3RouteTieWaves * 4;
  if (override_per_cu > 0) per_cu = override_per_cu < kN3RouteWaves * 4 ? override_per_cu : kN3RouteWaves * 4;
  return per_cu;
}

struct ChainRect {  // half-open cell rectangle
  int i0, j0, i1, j1;
};

enum ChainFilter { kFilterSlope = 1, kFilterStep = 2, kFilterRoughness = 3, kFilterCombine = 4, kFilterNormals = 5 };  // TE_FILTER_*

struct ChainRouteIn {
  DiscSummary normals, rough, step1, step2;  // disc_summary (te_disc.h)
  bool same_rough_disc = true;
  int axis = 2;
  double res = 0.05;
  int rows = 0, cols = 0, batch = 1;
  bool whole = true;          // every cell of every map; else `region` of one map (non-empty)
  ChainRect region = {0, 0, 0, 0};
  bool keep_normals = false, normals_only = false, generic_kernels = false, defer_combine = false;  // TE_RUN_*, kDeferCombine
  bool aux_stream = false;    // the shim hands a second stream (from 2^21 cells on, not under TE_RUN_SEQUENTIAL)
  bool raster = false;        // TE_OPT_NORMALS_ALGORITHM = 1: NormalVectorsFilter's raster method (whole maps only)
  bool sparse_holes = false, no_holes = false, skip_clean = false, short_strips = false, hole_queue = false;  // Layers' hints
  bool clip_table = true, tie_scratch = true, block_flags = true;
  bool guard_rows_elev = true, guard_rows_step_height = true;  // layer_has_guard_rows
  int cus = 256;
  // measurement switches of the lab build (TE_NO_SMALL, TE_SMALL_MAX_CELLS, TE_NO_CHAIN_WINDOW, TE_NO_N3, TE_N3_NO_TIES,
  // TE_N3_NO_SLIM, TE_N3_BLOCKS_PER_CU, TE_N3_EDGE_PERCENT, TE_N3_STRIP_ROWS, TE_STEP_NO_SMALL, TE_STEP_NO_TIES); the
  // defaults are the shipped library's
  bool no_small = false, no_chain_window = false, no_n3 = false, n3_no_ties = false, n3_no_slim = false, step_no_small = false,
       step_no_ties = false;
  int small_max_cells = 0, n3_blocks_per_cu = 0, n3_edge_percent = 50, n3_strip_rows = 0;
};

enum WholeKind { kWholeNone, kWholeChainWindow, kWholeNormalsSmall };  // k_chain_window | k_normals_small writing step and combine
enum StepKind { kStepSmall, kStepMarch, kStepMarchTies, kStepGeneric, kStepAny };
enum NormalsKind {
  kNormalsSmall, kNormals3Slim, kNormals3Sparse, kNormals3Dense, kNormals3Ties, kNormalsSlideShape, kNormalsSlideRadius, kNormalsGeneric,
  kNormalsAny, kNormalsNone, kNormalsRaster
};
enum CombineKind { kCombineNone, kCombineInNormals, kCombineKernel, kCombineDeferred, kCombineInChain };

struct StepRoute {
  StepKind kind = kStepGeneric;
  int Q = -1;  // the marches: the shape they are instantiated for (MarchTies: the disc without its circle, RAW)
};

// the strip plan of k_normals3* (te_n3_plan.h), computed once: the launcher copies these fields into the kernel's arguments
#define TE_N3_STRIP_FIELDS(X) X(rows) X(i_lo) X(i_hi) X(j_lo) X(j_hi) X(nbx) X(edge0) X(edge1) X(n_int) X(s_int) X(s_edge) X(rows_int) X(rows_edge) X(n_top) X(jf_lo) X(jf_hi)
struct N3Strips {
#define X(f) int f = 0;
  TE_N3_STRIP_FIELDS(X)
#undef X
};

struct ChainRoute {
  WholeKind whole = kWholeNone;
  StepRoute step_height, step_score;
  NormalsKind normals = kNormalsNone;
  bool cross = false;     // k_normals_small: the CROSS instantiation (the one-cell tie radius)
  bool keep = false;      // the normals kernel writes the normal layers
  bool fixup = false;     // k_normals_fixup follows
  // raster (normals == kNormalsRaster): k_normals_raster writes the normals, and the slope with `raster_slope`; the roughness
  // stage behind it reads those normals on the route TE_FILTER_ROUGHNESS takes (kNormalsNone: no roughness stage)
  bool raster_slope = false;
  NormalsKind rough = kNormalsNone;
  bool rough_fixup = false;
  CombineKind combine = kCombineNone;
  bool two_streams = false;
  bool steps = false;     // the step filter runs (not inside a one-kernel chain, not under normals only)
  // k_normals3*: the shape and radius it slides, the strip plan and its inputs
  int n3_shape = 0, n3_R = 0, n3_resident = 0, n3_blocks = 0;
  bool n3_short_strips = false;
  N3Strips n3;
  // the cells every stage covers: the region grown by the first step window, by both, by the normals reach, by the chain's
  ChainRect r_step1 = {0, 0, 0, 0}, r_step2 = {0, 0, 0, 0}, r_normals = {0, 0, 0, 0}, r_combine = {0, 0, 0, 0};
};

namespace route_detail {

inline ChainRect grown(const ChainRouteIn& in, int k) {
  if (in.whole) return ChainRect{0, 0, in.rows, in.cols};
  const ChainRect& r = in.region;
  return ChainRect{r.i0 - k < 0 ? 0 : r.i0 - k, r.j0 - k < 0 ? 0 : r.j0 - k, r.i1 + k > in.rows ? in.rows : r.i1 + k, r.j1 + k > in.cols ? in.cols : r.j1 + k};
}
inline int maps_of(const ChainRouteIn& in) { return in.whole ? in.batch : 1; }
inline long long cells_of(const ChainRouteIn& in, const ChainRect& r) { return (long long)(r.i1 - r.i0) * (r.j1 - r.j0) * maps_of(in); }
inline bool under_4gib(const ChainRouteIn& in) { return (double)in.rows * (double)in.cols * 4.0 < 4294967296.0; }  // 32-bit byte offsets inside a map
inline bool holds_disc(const ChainRouteIn& in, int R) { return in.rows >= 2 * R + 1 && in.cols >= 2 * R + 1; }     // never both borders inside one disc
inline bool any_disc(const ChainRouteIn& in) { return in.normals.any || in.rough.any || in.step1.any || in.step2.any; }

// One pass of the step filter on rectangle r; guard: its input layer has the slab's guard rows
inline StepRoute plan_step(const ChainRouteIn& in, const DiscSummary& d, const ChainRect& r, bool guard) {
  if (d.any) return StepRoute{kStepAny, -1};
  if (in.generic_kernels) return StepRoute{kStepGeneric, -1};
  // the marches: blocks 64 cells wide that never mask a lane, rows loaded beyond the layer
  const bool march_ok = guard && r.i1 - r.i0 >= kN3Lanes;
  if (d.n_ties == 0) {
    if (!in.step_no_small && d.Q == 0) return StepRoute{kStepSmall, -1};  // the centre alone
    if (march_ok && disc_shape(d.Q)) return StepRoute{kStepMarch, d.Q};
    return StepRoute{kStepGeneric, -1};
  }
  if (in.step_no_ties) return StepRoute{kStepGeneric, -1};
  if (!in.step_no_small && d.reach <= 2 && d.n_offsets <= kSmallOffsets) return StepRoute{kStepSmall, -1};  // a tie radius of one or two cells
  if (in.tie_scratch && march_ok && d.R >= 1 && d.ties_on_circle && step_raw_shape(d.q_runs)) return StepRoute{kStepMarchTies, d.q_runs};
  return StepRoute{kStepGeneric, -1};
}

// k_normals_small on rectangle r: discs that reach at most two cells; tie-free ones on small launches only
inline bool small_ok(const ChainRouteIn& in, const ChainRect& r) {
  const DiscSummary& d = in.normals;
  const long long small_launch = in.small_max_cells > 0 ? in.small_max_cells : kSmallLaunchCells;
  return !in.no_small && d.reach >= 1 && d.reach <= 2 && under_4gib(in) && (d.n_ties != 0 || cells_of(in, r) <= small_launch) &&
         d.n_offsets >= 2 && d.n_offsets <= kSmallOffsets;
}
inline bool small_cross(const DiscSummary& d) { return d.npoints == 1 && d.n_ties == 4 && d.reach == 1 && d.ties_on_circle; }

// k_normals3* on rectangle r (false: the sliding kernel, or for a tie radius the generic one, serves)
inline bool plan_n3(const ChainRouteIn& in, const ChainRect& r, ChainRoute& o) {
  const DiscSummary& d = in.normals;
  const bool ties = d.n_ties != 0;
  if (in.no_n3 || (ties && (in.n3_no_ties || !d.ties_on_circle))) return false;
  // the shape the kernel slides: the disc, or for a tie radius the disc with its circle (the shape reach^2)
  const int R = ties ? d.reach : d.R, shape = ties ? R * R : d.Q;
  const long long points = (long long)d.npoints + d.n_ties;
  if (R < 1 || shape < 1 || points < 3 || !n3_shape(shape)) return false;
  if (r.i1 - r.i0 < kN3Lanes || !in.clip_table || !holds_disc(in, R) || !under_4gib(in)) return false;
  // NormalVectorsFilter's eigenvalue test would fail everywhere
  if (!(in.res * in.res * ((double)(d.sii_runs + d.sii_ties) / (double)points) > 1e-8)) return false;
  // the TIES march knows the circle's cells from R (te_tie_triple.h): the disc's own table must say the same
  if (ties && (R < 3 || d.n_gen != tie_triple_cells(R) || d.n_ties != 4 + d.n_gen)) return false;
  const bool slim = !ties && n3_slim_shape(shape) && in.no_holes && !in.keep_normals && !in.n3_no_slim;
  const int maps = maps_of(in);
  o.n3_shape = shape;
  o.n3_R = R;
  o.n3_resident = n3_resident_per_cu(R, slim, ties, in.n3_blocks_per_cu) * in.cus;
  // strips of 32 rows only when the upload counted invalid cells and the dense march serves them
  o.n3_short_strips = in.short_strips && !slim && !ties;
  o.n3 = N3Strips();
  o.n3.rows = in.rows;
  o.n3.i_lo = r.i0;
  o.n3.i_hi = r.i1;
  o.n3.j_lo = r.j0;
  o.n3.j_hi = r.j1;
  n3_plan_edges(o.n3, in.rows, R);
  o.n3_blocks = n3_plan_strips(o.n3, in.cols, R, o.n3_resident, maps, o.n3_short_strips, in.n3_edge_percent, in.n3_strip_rows, nullptr);
  // the sparse march indexes its queues by block and the scratch holds one per resident block of the device: a grid that
  // did not fit one round takes the dense march (the kernel that keeps the normals exists with the dense march only)
  const bool queues_fit = (long long)o.n3_blocks * (long long)(maps > 0 ? maps : 1) <= (long long)(kN3RouteWaves * 4) * (long long)in.cus;
  o.normals = ties ? kNormals3Ties : slim ? kNormals3Slim : (!in.keep_normals && in.sparse_holes && in.hole_queue && queues_fit) ? kNormals3Sparse : kNormals3Dense;
  return true;
}

// the normals stage on rectangle r; fused: the kernel may write the weighted sum (the step layer is complete before it starts)
inline void plan_normals(const ChainRouteIn& in, const ChainRect& r, bool fused, ChainRoute& o) {
  const DiscSummary& d = in.normals;
  o.keep = in.keep_normals;
  o.fixup = false;
  o.cross = false;
  bool combined = fused;  // the generic kernel, the route of any radius and the sliding kernel combine when asked
  if (in.normals.any || in.rough.any) {
    o.normals = kNormalsAny;
  } else if (in.generic_kernels || !in.same_rough_disc || in.axis != 2) {
    o.normals = kNormalsGeneric;
  } else if (small_ok(in, r)) {
    o.normals = kNormalsSmall;
    o.cross = small_cross(d);
    combined = false;
  } else if (plan_n3(in, r, o)) {
    o.fixup = true;  // the frame and whatever the march flagged
    combined = false;
  } else if (d.n_ties == 0 && slide_radius(d.R) && d.npoints >= 3 && holds_disc(in, d.R) && in.clip_table) {
    o.normals = d.Q >= 1 && disc_shape(d.Q) ? kNormalsSlideShape : kNormalsSlideRadius;
    o.fixup = true;
  } else {
    o.normals = kNormalsGeneric;
  }
  // with the footprint pass right behind, its mask kernel (which reads the three scores anyway) combines
  o.combine = in.normals_only ? kCombineNone : in.defer_combine ? kCombineDeferred : combined ? kCombineInNormals : kCombineKernel;
}

// RoughnessFilter on given normals (TE_FILTER_ROUGHNESS, and the roughness stage of a raster chain), whole maps: the sliding
// kernel + fix-up for a tie-free disc, the generic kernel, or the route of any radius
inline void plan_given_roughness(const ChainRouteIn& in, NormalsKind& kind, bool& fixup) {
  const DiscSummary& d = in.rough;
  fixup = false;
  if (d.any)
    kind = kNormalsAny;
  else if (!in.generic_kernels && d.n_ties == 0 && slide_radius(d.R) && d.npoints >= 3 && in.block_flags && holds_disc(in, d.R)) {
    kind = d.Q >= 1 && disc_shape(d.Q) ? kNormalsSlideShape : kNormalsSlideRadius;
    fixup = true;
  } else
    kind = kNormalsGeneric;
}

// The chain under the raster method, whole maps (a region run is refused by the shim: normals stays kNormalsNone, which no
// launcher takes).  Never a one-kernel route; the normal layers are always written, roughness reads them.
inline void plan_raster(const ChainRouteIn& in, ChainRoute& o) {
  o.two_streams = in.aux_stream && !in.normals_only;
  o.steps = !in.normals_only;
  if (o.steps) {
    o.step_height = plan_step(in, in.step1, o.r_step1, in.guard_rows_elev);
    o.step_score = plan_step(in, in.step2, o.r_step2, in.guard_rows_step_height);
  }
  o.normals = kNormalsRaster;
  o.keep = true;
  o.raster_slope = !in.normals_only;
  if (!in.normals_only) plan_given_roughness(in, o.rough, o.rough_fixup);
  o.combine = in.normals_only ? kCombineNone : in.defer_combine ? kCombineDeferred : kCombineKernel;
}

inline void plan_rects(const ChainRouteIn& in, ChainRoute& o) {
  const int kn = in.normals.reach > in.rough.reach ? in.normals.reach : in.rough.reach, ks = in.step1.reach + in.step2.reach;
  o.r_step1 = grown(in, in.step1.reach);
  o.r_step2 = grown(in, ks);
  o.r_normals = grown(in, kn);
  o.r_combine = grown(in, kn > ks ? kn : ks);
}

}  // namespace route_detail

inline ChainRoute plan_chain_route(const ChainRouteIn& in) {
  using namespace route_detail;
  ChainRoute o;
  plan_rects(in, o);
  if (in.raster) {
    if (in.whole) plan_raster(in, o);
    return o;
  }
  const DiscSummary& d = in.normals;
  // A whole-map launch in ONE kernel (a disc marked `any` takes te_filter_any.hip for its own stage: none of these)
  if (in.whole && !in.generic_kernels && !any_disc(in) && !in.normals_only && in.same_rough_disc && in.axis == 2) {
    const bool tie_free_steps = in.step1.n_ties == 0 && in.step2.n_ties == 0;
    // k_chain_window: at most 2^18 cells, a normals disc that reaches at most two cells, step windows of at most 3 x 3
    if (!in.no_chain_window && d.reach >= 1 && d.reach <= 2 && tie_free_steps && in.step1.Q >= 0 && in.step1.Q <= 2 && in.step2.Q >= 0 &&
        in.step2.Q <= 2 && cells_of(in, o.r_normals) <= kSmallLaunchCells && under_4gib(in) && (long long)d.npoints + d.n_ties >= 3)
      o.whole = kWholeChainWindow;
    // single-cell step windows (score 1 where the elevation is valid): k_normals_small writes the step layer and the sum too
    else if (tie_free_steps && in.step1.Q == 0 && in.step2.Q == 0 && small_ok(in, o.r_normals))
      o.whole = kWholeNormalsSmall;
    if (o.whole != kWholeNone) {
      o.keep = in.keep_normals;
      o.cross = o.whole == kWholeNormalsSmall && small_cross(d);
      o.combine = in.defer_combine ? kCombineDeferred : kCombineInChain;
      return o;
    }
  }
  // The step filter and the normals kernel are independent until the combine: on whole maps they run on two streams
  o.two_streams = in.whole && in.aux_stream && !in.normals_only;
  o.steps = !in.normals_only;
  if (o.steps) {
    o.step_height = plan_step(in, in.step1, o.r_step1, in.guard_rows_elev);
    o.step_score = plan_step(in, in.step2, o.r_step2, in.guard_rows_step_height);
  }
  // the combine is fused into the normals kernel only when the step layer is complete before it starts (region runs: the
  // step reach may exceed the normals reach)
  plan_normals(in, o.r_normals, in.whole && !o.two_streams && !in.normals_only && !in.defer_combine, o);
  return o;
}

// One reference plugin at a time (launch_filter): always the whole maps.  TE_FILTER_STEP fills the two step routes,
// TE_FILTER_ROUGHNESS `normals` (given normals: the sliding kernel + fix-up, the generic kernel, or any radius),
// TE_FILTER_NORMALS is the chain plan with the roughness disc set to the normals disc, normals kept, normals only (under
// raster: k_normals_raster alone).
inline ChainRoute plan_filter_route(const ChainRouteIn& in0, int filter) {
  using namespace route_detail;
  ChainRouteIn in = in0;
  in.whole = true;
  if (filter == kFilterNormals) {
    in.rough = in.normals;
    in.same_rough_disc = true;
    in.keep_normals = in.normals_only = true;
    in.defer_combine = false;
    return plan_chain_route(in);
  }
  ChainRoute o;
  plan_rects(in, o);
  if (filter == kFilterStep) {
    o.steps = true;
    o.step_height = plan_step(in, in.step1, o.r_step1, in.guard_rows_elev);
    o.step_score = plan_step(in, in.step2, o.r_step2, in.guard_rows_step_height);
  } else if (filter == kFilterRoughness) {
    o.keep = true;
    plan_given_roughness(in, o.normals, o.fixup);
  } else if (filter == kFilterCombine) {
    o.combine = kCombineKernel;
  }
  return o;
}

}  // namespace fast
}  // namespace te
