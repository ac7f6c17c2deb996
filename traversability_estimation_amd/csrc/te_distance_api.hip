// te_distance_api.hip -- C-ABI of te_run_distance / te_run_distance_region / te_distance_stats / te_time_distance_samples
// (include/travgpu.h: the clearance layer).  The plan: te_distance_plan.h; the kernels: te_distance.hip; the per-cell routines:
// te_distance.h.  The context: te_ctx.h.
#include "te_ctx.h"
#include "te_distance_launch.h"

using namespace te;
using namespace te::shim;

static_assert(TE_DISTANCE_BELOW == distance::kBelow && TE_DISTANCE_ABOVE == distance::kAbove && TE_DISTANCE_NAN_IS_SEED == distance::kNanIsSeed,
              "te_distance.h restates the modes of travgpu.h");

namespace {

// the arguments that need no context; timing: te_time_distance_samples also takes mode 0 and the two pass bits
int check_args(const char* who, int mode, double threshold, double max_distance, bool timing) {
  const int kind = mode & ~(TE_DISTANCE_NAN_IS_SEED | (timing ? TE_DISTANCE_TIME_PASS1 | TE_DISTANCE_TIME_PASS2 : 0));
  if (!(kind == TE_DISTANCE_BELOW || kind == TE_DISTANCE_ABOVE || (timing && mode == 0)))
    return fail(TE_ERR_INVALID_ARG, "%s: mode %d is neither TE_DISTANCE_BELOW nor TE_DISTANCE_ABOVE (with or without TE_DISTANCE_NAN_IS_SEED)", who, mode);
  if (!isfinite(threshold)) return fail(TE_ERR_BAD_PARAM, "%s: threshold must be finite", who);
  if (!(max_distance > 0.0) || !isfinite(max_distance)) return fail(TE_ERR_BAD_PARAM, "%s: max_distance must be finite and positive", who);
  return TE_OK;
}

// the cap in cells at the context's resolution (the geometry is set)
int cap_cells(const char* who, const te_ctx* c, double max_distance, uint32_t* cap2, int* R) {
  if (!distance::cap_of(max_distance, c->geo.res, cap2, R))
    return fail(TE_ERR_BAD_PARAM, "%s: max_distance %g is more than %d cells of %g m", who, max_distance, distance::kMaxReach, c->geo.res);
  return TE_OK;
}

// the plan's grids and the scratch of pass 1 for `nmaps` maps
int scratch(const char* who, te_ctx* c, const distance::Plan& p, int nmaps, distance::Args* a) {
  if (!p.fits) return fail(TE_ERR_UNSUPPORTED, "%s: a map of %d x %d cells is more than one launch takes", who, p.rows, p.cols);
  if (const int rc = reserve_scratch(who, c->lmem.distance_g, p.g_cells * (size_t)nmaps * sizeof(uint16_t), c->stream, "the column distances")) return rc;
  a->g = c->lmem.distance_g.as<uint16_t>();
  return TE_OK;
}

void fill_args(const te_ctx* c, int mode, double threshold, double max_distance, int nmaps, distance::Args* a) {
  a->nmaps = nmaps;
  a->mode = mode & (TE_DISTANCE_BELOW | TE_DISTANCE_ABOVE | TE_DISTANCE_NAN_IS_SEED);
  a->threshold = (float)threshold;
  a->res = c->geo.res;
  a->beyond = (float)max_distance;
}

// checks, scratch and plan of a whole-map call; caller holds the lock and has made the device current
int prepare(const char* who, te_ctx* c, int mode, double threshold, double max_distance, int in_layer, int out_layer, int map0, int nmaps, distance::Plan* plan,
            distance::Args* a) {
  CallWhere at;
  at.map0 = map0, at.nmaps = nmaps, at.max_maps = 65535;
  if (const int rc = refused(who, c, layer_call::check(facts_of(c), in_layer, out_layer, map0, nmaps, at.max_maps), at)) return rc;
  uint32_t cap2 = 0;
  int R = 0;
  if (const int rc = cap_cells(who, c, max_distance, &cap2, &R)) return rc;
  const int rows = c->geo.rows, cols = c->geo.cols;
  *plan = distance::plan(rows, cols, cap2, R, c->opt_distance_route, region::Rect{0, 0, rows, cols});
  if (const int rc = scratch(who, c, *plan, nmaps, a)) return rc;
  // (in place needs no copy: pass 1 leaves nothing of the input to read)
  if (in_layer != out_layer)
    if (const int rc = ensure_input_layer(c, out_layer)) return rc;
  const size_t cells = (size_t)rows * cols;
  a->in = layer_ptr(c, in_layer) + cells * map0;
  a->out = layer_ptr(c, out_layer) + cells * map0;
  fill_args(c, mode, threshold, max_distance, nmaps, a);
  return TE_OK;
}

}  // namespace

extern "C" {

int te_run_distance(te_ctx* c, int mode, double threshold, double max_distance, int in_layer, int out_layer, int map0, int nmaps) {
  const char* const who = "te_run_distance";
  if (!c) return fail(TE_ERR_INVALID_ARG, "%s: NULL", who);
  if (const int rc = check_args(who, mode, threshold, max_distance, false)) return rc;
  TraceRange tr(who);
  CtxLock lk(c, /*beside_prefetch*/ true, bit(in_layer) | bit(out_layer));
  if (c->have_geo) HIP_TRY(hipSetDevice(c->device));
  distance::Plan plan;
  distance::Args a{};
  if (const int rc = prepare(who, c, mode, threshold, max_distance, in_layer, out_layer, map0, nmaps, &plan, &a)) return rc;
  c->distance_counts_valid = false;
  HIP_TRY(distance::launch(plan, a, distance::kBothPasses, c->stream, c->distance_counts));
  c->distance_counts_valid = true;
  return note_layer_written(c, out_layer);
}

int te_run_distance_region(te_ctx* c, int mode, double threshold, double max_distance, int in_layer, int out_layer, int map, int row0, int col0, int h, int w,
                           int out_rect[4]) {
  const char* const who = "te_run_distance_region";
  if (!c || !out_rect) return fail(TE_ERR_INVALID_ARG, "%s: NULL", who);
  if (const int rc = check_args(who, mode, threshold, max_distance, false)) return rc;
  TraceRange tr(who);
  CtxLock lk(c, /*beside_prefetch*/ true, bit(in_layer) | bit(out_layer));
  if (c->have_geo) HIP_TRY(hipSetDevice(c->device));
  // (the order of the whole-map call: the layers and the rectangle, then the cap, which needs the resolution; nothing is
  // touched before every check has passed)
  CallWhere at;
  at.map0 = map, at.row0 = row0, at.col0 = col0, at.h = h, at.w = w;
  if (const int rc = refused(who, c, layer_call::check_region(facts_of(c), in_layer, out_layer, map, row0, col0, h, w), at)) return rc;
  uint32_t cap2 = 0;
  int R = 0;
  if (const int rc = cap_cells(who, c, max_distance, &cap2, &R)) return rc;
  distance::Args a{};
  if (const int rc = region_filter_layers(who, c, in_layer, out_layer, map, row0, col0, h, w, &a.in, &a.out)) return rc;
  const distance::Plan plan = distance::plan(c->geo.rows, c->geo.cols, cap2, R, c->opt_distance_route, region::Rect{row0, col0, row0 + h, col0 + w});
  if (const int rc = scratch(who, c, plan, 1, &a)) return rc;
  fill_args(c, mode, threshold, max_distance, 1, &a);
  c->distance_counts_valid = false;
  HIP_TRY(distance::launch(plan, a, distance::kBothPasses, c->stream, c->distance_counts));
  c->distance_counts_valid = true;
  write_rect(plan.out, out_rect);
  note_region_written(c, out_layer);
  return TE_OK;
}

int te_distance_stats(te_ctx* c, uint64_t counts[2]) {
  if (!c || !counts) return fail(TE_ERR_INVALID_ARG, "te_distance_stats: NULL");
  CtxLock lk(c);
  if (!c->distance_counts_valid) return fail(TE_ERR_NOT_READY, "te_distance_stats: no te_run_distance has run on this context");
  counts[0] = c->distance_counts[0];
  counts[1] = c->distance_counts[1];
  return TE_OK;
}

int te_time_distance_samples(te_ctx* c, int mode, double threshold, double max_distance, int in_layer, int out_layer, int warmup, int iters, float* ms) {
  const char* const who = "te_time_distance_samples";
  if (!c || !ms || iters <= 0 || warmup < 0) return fail(TE_ERR_INVALID_ARG, "%s: bad argument", who);
  if (in_layer == out_layer) return fail(TE_ERR_INVALID_ARG, "%s: the input layer must survive the repeats (in_layer == out_layer)", who);
  if (const int rc = check_args(who, mode, threshold, max_distance, true)) return rc;
  CtxLock lk(c);
  if (c->have_geo) HIP_TRY(hipSetDevice(c->device));
  distance::Plan plan;
  distance::Args a{};
  const bool copy = mode == 0;
  if (const int rc = prepare(who, c, copy ? TE_DISTANCE_BELOW : mode, threshold, max_distance, in_layer, out_layer, 0, c->have_geo ? c->geo.batch : 1, &plan, &a))
    return rc;
  int passes = (mode & TE_DISTANCE_TIME_PASS1 ? distance::kPass1 : 0) | (mode & TE_DISTANCE_TIME_PASS2 ? distance::kPass2 : 0);
  if (!passes) passes = distance::kBothPasses;
  const size_t bytes = (size_t)c->geo.rows * c->geo.cols * (size_t)c->geo.batch * sizeof(float);
  c->distance_counts_valid = false;
  // (pass 2 alone reads what a pass 1 left)
  if (!copy && passes == distance::kPass2) HIP_TRY(distance::launch(plan, a, distance::kPass1, c->stream, nullptr));
  const auto nothing = []() -> int { return TE_OK; };
  const auto body = [&]() -> int {
    if (copy)
      HIP_TRY(hipMemcpyAsync(a.out, a.in, bytes, hipMemcpyDeviceToDevice, c->stream));
    else
      HIP_TRY(distance::launch(plan, a, passes, c->stream, c->distance_counts));
    return TE_OK;
  };
  if (const int rc = time_samples(c, /*locked*/ true, warmup, iters, ms, nothing, body)) return rc;
  c->distance_counts_valid = !copy && (passes & distance::kPass2);
  // out_layer now holds the result, the copy, or (pass 1 alone) what it held: the facts of an upload of those values
  return note_layer_written(c, out_layer);
}

}  // extern "C"
