// te_components_api.hip -- C-ABI of te_run_components / te_run_reachable / te_components_stats (include/travgpu.h: the connected
// regions of the free cells).  The plan: te_components_plan.h; the kernels: te_components.hip; the per-run and union routines:
// te_components.h.  The context: te_ctx.h.
#include "te_components_launch.h"
#include "te_ctx.h"
#include "te_distance.h"

using namespace te;
using namespace te::shim;

static_assert(TE_REACHABLE_MAX_STARTS == components::kMaxStarts, "te_components_plan.h restates the limit of travgpu.h");
static_assert(TE_COMPONENTS_CONNECTIVITY_4 == 4 && TE_COMPONENTS_CONNECTIVITY_8 == 8, "the connectivity is the number of neighbours");

namespace {

// the arguments that need no context
int check_args(const char* who, int mode, double threshold, int connectivity) {
  const int kind = mode & ~TE_DISTANCE_NAN_IS_SEED;
  if (!(kind == TE_DISTANCE_BELOW || kind == TE_DISTANCE_ABOVE))
    return fail(TE_ERR_INVALID_ARG, "%s: mode %d is neither TE_DISTANCE_BELOW nor TE_DISTANCE_ABOVE (with or without TE_DISTANCE_NAN_IS_SEED)", who, mode);
  if (!(connectivity == TE_COMPONENTS_CONNECTIVITY_4 || connectivity == TE_COMPONENTS_CONNECTIVITY_8))
    return fail(TE_ERR_INVALID_ARG, "%s: connectivity %d is neither 4 nor 8", who, connectivity);
  if (!isfinite(threshold)) return fail(TE_ERR_BAD_PARAM, "%s: threshold must be finite", who);
  return TE_OK;
}

// checks, plan and scratch of a call; caller holds the lock and has made the device current.  Nothing is touched before every
// check has passed (n_starts == 0: te_run_components).
int prepare(const char* who, te_ctx* c, int mode, double threshold, int connectivity, int in_layer, int out_layer, int map0, int nmaps, int n_starts,
            const int* start_cells, components::Plan* plan, components::Args* a, components::Starts* starts) {
  CallWhere at;
  at.map0 = map0, at.nmaps = nmaps, at.max_maps = 65535;
  if (const int rc = refused(who, c, layer_call::check(facts_of(c), in_layer, out_layer, map0, nmaps, at.max_maps), at)) return rc;
  const int rows = c->geo.rows, cols = c->geo.cols;
  starts->n = n_starts;
  for (int k = 0; k < n_starts; ++k) {
    const int row = start_cells[2 * k], col = start_cells[2 * k + 1];
    if (row < 0 || row >= rows || col < 0 || col >= cols)
      return fail(TE_ERR_INVALID_ARG, "%s: start %d, cell (%d, %d), lies outside the map of %d x %d cells", who, k, row, col, rows, cols);
    starts->cell[k] = (uint32_t)((size_t)col * (size_t)rows + (size_t)row);
  }
  *plan = components::plan(rows, cols, nmaps);
  if (!plan->fits) return fail(TE_ERR_UNSUPPORTED, "%s: a map of %d x %d cells is more than the 32-bit labels take (2^31 cells)", who, rows, cols);
  if (const int rc = reserve_scratch(who, c->lmem.components_scratch, plan->scratch_bytes, c->stream, "the labels and counts")) return rc;
  if (c->cmem.components_counts.once(4 * sizeof(unsigned long long)) != hipSuccess)
    return fail(TE_ERR_UNSUPPORTED, "%s: the four totals do not fit in device memory", who);
  // (in place needs no copy: the tile pass leaves nothing of the input to read)
  if (in_layer != out_layer)
    if (const int rc = ensure_input_layer(c, out_layer)) return rc;
  const size_t cells = (size_t)rows * cols;
  a->in = layer_ptr(c, in_layer) + cells * map0;
  a->out = layer_ptr(c, out_layer) + cells * map0;
  a->scratch = c->lmem.components_scratch.p;
  a->counts = c->cmem.components_counts.as<unsigned long long>();
  a->nmaps = nmaps;
  a->mode = mode & (TE_DISTANCE_BELOW | TE_DISTANCE_ABOVE | TE_DISTANCE_NAN_IS_SEED);
  a->threshold = (float)threshold;
  a->connectivity = connectivity;
  return TE_OK;
}

int run(const char* who, te_ctx* c, int mode, double threshold, int connectivity, int in_layer, int out_layer, int map0, int nmaps, int n_starts,
        const int* start_cells) {
  TraceRange tr(who);
  CtxLock lk(c, /*beside_prefetch*/ true, bit(in_layer) | bit(out_layer));
  if (c->have_geo) HIP_TRY(hipSetDevice(c->device));
  components::Plan plan;
  components::Args a{};
  components::Starts starts;
  if (const int rc = prepare(who, c, mode, threshold, connectivity, in_layer, out_layer, map0, nmaps, n_starts, start_cells, &plan, &a, &starts)) return rc;
  c->components_counts_valid = false;
  HIP_TRY(components::launch(plan, a, n_starts ? &starts : nullptr, c->stream));
  c->components_counts_valid = true;
  return note_layer_written(c, out_layer);
}

}  // namespace

extern "C" {

int te_run_components(te_ctx* c, int mode, double threshold, int connectivity, int in_layer, int out_layer, int map0, int nmaps) {
  const char* const who = "te_run_components";
  if (const int rc = check_args(who, mode, threshold, connectivity)) return rc;
  if (!c) return fail(TE_ERR_INVALID_ARG, "%s: NULL", who);
  return run(who, c, mode, threshold, connectivity, in_layer, out_layer, map0, nmaps, 0, nullptr);
}

int te_run_reachable(te_ctx* c, int mode, double threshold, int connectivity, int in_layer, int out_layer, int map, int n_starts, const int* start_cells) {
  const char* const who = "te_run_reachable";
  if (const int rc = check_args(who, mode, threshold, connectivity)) return rc;
  if (n_starts < 1 || n_starts > TE_REACHABLE_MAX_STARTS)
    return fail(TE_ERR_INVALID_ARG, "%s: n_starts %d is not in [1, %d]", who, n_starts, TE_REACHABLE_MAX_STARTS);
  if (!start_cells) return fail(TE_ERR_INVALID_ARG, "%s: start_cells is NULL", who);
  if (!c) return fail(TE_ERR_INVALID_ARG, "%s: NULL", who);
  return run(who, c, mode, threshold, connectivity, in_layer, out_layer, map, 1, n_starts, start_cells);
}

int te_components_stats(te_ctx* c, uint64_t counts[4]) {
  if (!c || !counts) return fail(TE_ERR_INVALID_ARG, "te_components_stats: NULL");
  CtxLock lk(c);
  if (!c->components_counts_valid) return fail(TE_ERR_NOT_READY, "te_components_stats: no te_run_components or te_run_reachable has run on this context");
  HIP_TRY(hipSetDevice(c->device));
  unsigned long long h[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(h, c->cmem.components_counts.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int k = 0; k < 4; ++k) counts[k] = h[k];
  return TE_OK;
}

}  // extern "C"
