// te_radius_api.hip -- C-ABI of te_run_radius_filter / te_radius_filter_stats (include/travgpu.h: MeanInRadiusFilter and
// MinInRadiusFilter on the device).  The plan and the predicate: te_radius_plan.h; the kernels: te_radius.hip; the disc:
// te_disc_table.h.  The context: te_ctx.h.
#include "te_ctx.h"
#include "te_radius_launch.h"

using namespace te;
using namespace te::shim;

namespace {

struct Call {
  radius::Window w;
  radius::Args a;
  radius::Plan plan;
};

// the window table of (radius, resolution) on the device: built and uploaded when the last call's was another one
int window_table(const char* who, te_ctx* c, double rad, radius::Window* w, radius::Shape* shape) {
  const double res = c->geo.res;
  if (!(c->radius_tab_radius == rad && c->radius_tab_res == res && c->cmem.radius_tab.p)) {
    // (an upload of the table before may still read the host copy)
    if (!c->radius_tab_host.empty()) HIP_TRY(hipStreamSynchronize(c->stream));
    c->radius_tab_radius = -1.0;
    DiscTable& t = c->radius_disc;
    build_disc_table(rad, res, &t);
    std::vector<int32_t>& h = c->radius_tab_host;
    h.assign(t.hw.begin(), t.hw.end());
    // the ties in the contract's order: row offset ascending, then column offset ascending
    std::vector<std::pair<int32_t, int32_t>> ties;
    for (int k = 0; k < t.n_ties(); ++k) ties.emplace_back(t.ties[2 * (size_t)k], t.ties[2 * (size_t)k + 1]);
    std::sort(ties.begin(), ties.end());
    for (const auto& q : ties) h.push_back(q.first), h.push_back(q.second);
    if (h.empty()) h.push_back(0);  // (never: a disc without a run has its centre as a tie)
    if (const int rc = reserve_scratch(who, c->cmem.radius_tab, h.size() * sizeof(int32_t), c->stream, "the window table")) return rc;
    HIP_TRY(hipMemcpyAsync(c->cmem.radius_tab.p, h.data(), h.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    c->radius_tab_radius = rad;
    c->radius_tab_res = res;
  }
  const DiscTable& t = c->radius_disc;
  w->tab = c->cmem.radius_tab.as<int32_t>();
  w->r2 = t.r2;
  w->R = t.R;
  w->hw0 = t.R >= 0 ? t.hw[0] : 0;
  w->reach = t.reach;
  w->n_ties = t.n_ties();
  shape->R = w->R;
  shape->hw0 = w->hw0;
  shape->reach = w->reach;
  shape->n_ties = w->n_ties;
  shape->npoints = t.npoints;
  return TE_OK;
}

// checks, scratch and plan of one call; caller holds the lock and has made the device current.  With in_layer == out_layer
// the kernels read a copy of the input, queued here.
int prepare(const char* who, te_ctx* c, int op, double rad, int in_layer, int out_layer, int map0, int nmaps, Call* call) {
  CallWhere at;
  at.map0 = map0, at.nmaps = nmaps, at.max_maps = 65535;
  if (const int rc = refused(who, c, layer_call::check(facts_of(c), in_layer, out_layer, map0, nmaps, at.max_maps), at)) return rc;
  if (in_layer != out_layer)
    if (const int rc = ensure_input_layer(c, out_layer)) return rc;  // (robot_slope exists from its first write on)
  const float* const in = layer_ptr(c, in_layer);
  float* const out = layer_ptr(c, out_layer);

  const int rows = c->geo.rows, cols = c->geo.cols;
  const size_t cells = (size_t)rows * cols, total = cells * (size_t)nmaps;
  radius::Shape shape;
  if (const int rc = window_table(who, c, radius::bounded_radius(rad, c->geo.res, rows, cols), &call->w, &shape)) return rc;
  call->plan = radius::plan(op, rows, cols, shape, c->opt_radius_route);

  HIP_TRY(c->cmem.radius_counts.once(2 * sizeof(unsigned long long)));
  const float* in_first = in + cells * map0;  // the first map of the call
  if (in_layer == out_layer) {
    te::DevBuf& copy = c->lmem.radius_copy;
    if (const int rc = reserve_scratch(who, copy, c->layer_elems * sizeof(float), c->stream, "the copy of the input layer")) return rc;
    HIP_TRY(hipMemcpyAsync(copy.p, in_first, total * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    in_first = copy.as<float>();
  }
  call->a.in = in_first;
  call->a.out = out + cells * map0;
  call->a.counts = c->cmem.radius_counts.as<unsigned long long>();
  call->a.nmaps = nmaps;
  call->a.op = op;
  return TE_OK;
}

int check_args(const char* who, int op, double rad, bool copy_ok) {
  if (!(op == TE_RADIUS_MEAN || op == TE_RADIUS_MIN || (copy_ok && op == 0))) return fail(TE_ERR_INVALID_ARG, "%s: op %d is neither TE_RADIUS_MEAN nor TE_RADIUS_MIN", who, op);
  if (!(rad >= 0.0) || !isfinite(rad)) return fail(TE_ERR_BAD_PARAM, "%s: radius must be finite and not negative", who);
  return TE_OK;
}

}  // namespace

extern "C" {

int te_run_radius_filter(te_ctx* c, int op, double rad, int in_layer, int out_layer, int map0, int nmaps) {
  if (!c) return fail(TE_ERR_INVALID_ARG, "te_run_radius_filter: NULL");
  if (const int rc = check_args("te_run_radius_filter", op, rad, false)) return rc;
  TraceRange tr("te_run_radius_filter");
  // (bit() of an id out of range is 0: te_ctx_state.h, layer_bit; prepare refuses the id under the lock)
  CtxLock lk(c, /*beside_prefetch*/ true, bit(in_layer) | bit(out_layer));
  Call call{};
  if (c->have_geo) HIP_TRY(hipSetDevice(c->device));
  if (const int rc = prepare("te_run_radius_filter", c, op, rad, in_layer, out_layer, map0, nmaps, &call)) return rc;
  c->radius_counts_valid = false;
  HIP_TRY(hipMemsetAsync(call.a.counts, 0, 2 * sizeof(unsigned long long), c->stream));
  HIP_TRY(radius::launch(c->geo, call.w, call.a, call.plan, c->stream));
  c->radius_counts_valid = true;
  return note_layer_written(c, out_layer);
}

int te_run_radius_filter_region(te_ctx* c, int op, double rad, int in_layer, int out_layer, int map, int row0, int col0, int h, int w, int out_rect[4]) {
  const char* const who = "te_run_radius_filter_region";
  if (!c || !out_rect) return fail(TE_ERR_INVALID_ARG, "%s: NULL", who);
  if (const int rc = check_args(who, op, rad, false)) return rc;
  TraceRange tr(who);
  CtxLock lk(c, /*beside_prefetch*/ true, bit(in_layer) | bit(out_layer));
  if (c->have_geo) HIP_TRY(hipSetDevice(c->device));
  const float* in = nullptr;
  float* out = nullptr;
  if (const int rc = region_filter_layers(who, c, in_layer, out_layer, map, row0, col0, h, w, &in, &out)) return rc;
  const int rows = c->geo.rows, cols = c->geo.cols;
  // (the table of the last call with this radius and resolution is kept: nothing is rebuilt from tick to tick)
  Call call{};
  radius::Shape shape;
  if (const int rc = window_table(who, c, radius::bounded_radius(rad, c->geo.res, rows, cols), &call.w, &shape)) return rc;
  const region::Rect dirty = {row0, col0, row0 + h, col0 + w};
  const radius::RegionPlan plan = radius::region_plan(op, rows, cols, shape, c->opt_radius_route, dirty);
  HIP_TRY(c->cmem.radius_counts.once(2 * sizeof(unsigned long long)));
  call.a.in = in;
  call.a.out = out;
  call.a.counts = c->cmem.radius_counts.as<unsigned long long>();
  call.a.nmaps = 1;
  call.a.op = op;
  c->radius_counts_valid = false;
  HIP_TRY(hipMemsetAsync(call.a.counts, 0, 2 * sizeof(unsigned long long), c->stream));
  HIP_TRY(radius::launch_region(c->geo, call.w, call.a, plan, c->stream));
  c->radius_counts_valid = true;
  write_rect(plan.out, out_rect);
  note_region_written(c, out_layer);
  return TE_OK;
}

int te_radius_filter_stats(te_ctx* c, uint64_t counts[2]) {
  if (!c || !counts) return fail(TE_ERR_INVALID_ARG, "te_radius_filter_stats: NULL");
  CtxLock lk(c);
  if (!c->radius_counts_valid || !c->cmem.radius_counts.p) return fail(TE_ERR_NOT_READY, "te_radius_filter_stats: no te_run_radius_filter has run on this context");
  return read_block_counts(c, c->cmem.radius_counts, counts);
}

int te_time_radius_filter_samples(te_ctx* c, int op, double rad, int in_layer, int out_layer, int warmup, int iters, float* ms) {
  if (!c || !ms || iters <= 0 || warmup < 0) return fail(TE_ERR_INVALID_ARG, "te_time_radius_filter_samples: bad argument");
  if (in_layer == out_layer) return fail(TE_ERR_INVALID_ARG, "te_time_radius_filter_samples: the input layer must survive the repeats (in_layer == out_layer)");
  if (const int rc = check_args("te_time_radius_filter_samples", op, rad, true)) return rc;
  CtxLock lk(c);
  if (c->have_geo) HIP_TRY(hipSetDevice(c->device));
  Call call{};
  if (const int rc = prepare("te_time_radius_filter_samples", c, op ? op : TE_RADIUS_MIN, rad, in_layer, out_layer, 0, c->have_geo ? c->geo.batch : 1, &call)) return rc;
  const size_t bytes = (size_t)c->geo.rows * c->geo.cols * (size_t)c->geo.batch * sizeof(float);
  c->radius_counts_valid = false;
  const auto clear = [&]() -> int {
    HIP_TRY(hipMemsetAsync(call.a.counts, 0, 2 * sizeof(unsigned long long), c->stream));
    return TE_OK;
  };
  const auto body = [&]() -> int {
    if (op)
      HIP_TRY(radius::launch(c->geo, call.w, call.a, call.plan, c->stream));
    else
      HIP_TRY(hipMemcpyAsync(call.a.out, call.a.in, bytes, hipMemcpyDeviceToDevice, c->stream));
    return TE_OK;
  };
  if (const int rc = time_samples(c, /*locked*/ true, warmup, iters, ms, clear, body)) return rc;
  c->radius_counts_valid = op != 0;
  // out_layer now holds the result (or the copy): the facts of an upload of those values
  return note_layer_written(c, out_layer);
}

}  // extern "C"
