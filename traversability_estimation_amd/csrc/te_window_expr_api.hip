// te_window_expr_api.hip -- C-ABI of te_run_window_expression / te_window_expr_check / te_window_expression_stats
// (include/travgpu.h: gridMapFilters/SlidingWindowMathExpressionFilter on the device).  The language and its compiler:
// te_expr.h (compile_window); the plan: te_window_plan.h; the kernel: te_window_expr.hip.  The context: te_ctx.h.
#include "te_ctx.h"
#include "te_region_plan.h"
#include "te_window_expr_launch.h"

using namespace te;
using namespace te::shim;

static_assert(TE_EDGE_INSIDE == wexpr::kInside && TE_EDGE_CROP == wexpr::kCrop && TE_EDGE_EMPTY == wexpr::kEmpty && TE_EDGE_MEAN == wexpr::kMean,
              "te_window_plan.h restates TE_EDGE_*");
static_assert(wexpr::kStackSlots == expr::kMaxStack - 1 && wexpr::kResSlots == expr::kMaxRed, "te_window_plan.h restates the limits of te_expr.h");
static_assert(wexpr::kPartialBytes <= sizeof(expr::Partial), "a column Partial as arrays");

namespace {

struct Call {
  expr::Program prog;
  wexpr::Args a;
  wexpr::Plan plan;
};

// c: the context whose user layers are names too (a user in_layer is the window's variable; an id that is no layer is
// refused here, before the text), or NULL
int compile(const char* who, const char* text, int in_layer, expr::Program* p, te_ctx* c = nullptr) {
  char err[200];
  UserNames un;
  if (c) {
    snapshot_user_names(c, &un);
    layer_call::Facts ids;  // (the ids alone: the layers are judged under the lock)
    ids.user_added = un.copy.mask();
    if (!layer_call::known(ids, in_layer)) return refused(who, c, {TE_ERR_INVALID_ARG, layer_call::kBadInput, in_layer, false});
  }
  const int rc = expr::compile_window(text, in_layer, p, err, sizeof(err), un.v, un.n);
  return rc == TE_OK ? TE_OK : fail(rc, "%s: %s", who, err);
}

// the kernel's arguments: `in` / `out` at the first map of `nmaps`; after cmem.window_counts.once
void fill_args(te_ctx* c, const te_window_expr_params* p, const float* in, float* out, int nmaps, wexpr::Args* a) {
  a->in = in;
  a->out = out;
  a->counts = c->cmem.window_counts.as<unsigned long long>();
  a->rows = c->geo.rows;
  a->cols = c->geo.cols;
  a->nmaps = nmaps;
  a->edge = p->edge_handling;
  a->compute_empty_cells = p->compute_empty_cells != 0;
}

// checks, scratch and plan of one call; caller holds the lock and has made the device current.  With in_layer == out_layer
// the kernel reads a copy of the input, queued here.
int prepare(const char* who, te_ctx* c, const te_window_expr_params* p, int in_layer, int out_layer, int map0, int nmaps, Call* call) {
  CallWhere at;
  at.map0 = map0, at.nmaps = nmaps, at.max_maps = 65535;
  if (const int rc = refused(who, c, layer_call::check(facts_of(c), in_layer, out_layer, map0, nmaps, at.max_maps), at)) return rc;
  if (in_layer != out_layer)
    if (const int rc = ensure_input_layer(c, out_layer)) return rc;  // (robot_slope exists from its first write on)
  const float* const in = layer_ptr(c, in_layer);
  float* const out = layer_ptr(c, out_layer);

  const int rows = c->geo.rows, cols = c->geo.cols;
  int w = 0;
  if (const char* why = wexpr::window_from_params(p->window_size, p->use_window_length, p->window_length, c->geo.res, &w))
    return fail(TE_ERR_BAD_PARAM, "%s: %s", who, why);
  call->plan = wexpr::plan(rows, cols, w, call->prog.n_red, call->prog.n_outer, c->opt_window_expr_route);
  if (!call->plan.fits) return fail(TE_ERR_UNSUPPORTED, "%s: a map of %d x %d cells with a window of %d is more than the kernel indexes", who, rows, cols, w);

  const size_t cells = (size_t)rows * cols, total = cells * (size_t)nmaps;
  HIP_TRY(c->cmem.window_counts.once(2 * sizeof(unsigned long long)));
  const float* in_first = in + cells * map0;  // the first map of the call
  if (in_layer == out_layer) {
    te::DevBuf& copy = c->lmem.window_copy;
    if (const int rc = reserve_scratch(who, copy, c->layer_elems * sizeof(float), c->stream, "the copy of the input layer")) return rc;
    HIP_TRY(hipMemcpyAsync(copy.p, in_first, total * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    in_first = copy.as<float>();
  }
  fill_args(c, p, in_first, out + cells * map0, nmaps, &call->a);
  return TE_OK;
}

}  // namespace

extern "C" {

int te_window_expr_params_default(te_window_expr_params* p) {
  if (!p) return fail(TE_ERR_INVALID_ARG, "te_window_expr_params_default: NULL");
  memset(p, 0, sizeof(*p));
  p->size = (uint32_t)sizeof(te_window_expr_params);
  p->abi_version = TE_ABI_VERSION;
  // SlidingWindowMathExpressionFilter::configure(), as remembered (travgpu.h); upstream has no default window: 3 here
  p->window_size = 3;
  p->use_window_length = 0;
  p->window_length = 0.0;
  p->compute_empty_cells = 1;
  p->edge_handling = TE_EDGE_INSIDE;
  return TE_OK;
}

int te_window_expr_params_validate(const te_window_expr_params* p) {
  if (!p) return fail(TE_ERR_INVALID_ARG, "te_window_expr_params: NULL");
  if (p->size != sizeof(te_window_expr_params) || p->abi_version != TE_ABI_VERSION)
    return fail(TE_ERR_INVALID_ARG, "te_window_expr_params: size/abi mismatch (got %u/%u, want %zu/%d)", p->size, p->abi_version, sizeof(te_window_expr_params),
                TE_ABI_VERSION);
  if (p->use_window_length != 0 && p->use_window_length != 1)
    return fail(TE_ERR_BAD_PARAM, "SlidingWindowMathExpressionFilter: use_window_length is 0 (window_size) or 1 (window_length)");
  if (p->use_window_length && p->window_size != 0)
    return fail(TE_ERR_BAD_PARAM, "SlidingWindowMathExpressionFilter: exactly one of window_size and window_length (with window_length, window_size stays 0)");
  if (!p->use_window_length && p->window_length != 0.0)
    return fail(TE_ERR_BAD_PARAM, "SlidingWindowMathExpressionFilter: exactly one of window_size and window_length (with window_size, window_length stays 0)");
  if (p->use_window_length) {
    if (!(p->window_length >= 0.0) || !isfinite(p->window_length)) return fail(TE_ERR_BAD_PARAM, "SlidingWindowMathExpressionFilter: window_length must be finite and not negative");
  } else if (p->window_size < 1 || p->window_size % 2 == 0) {
    return fail(TE_ERR_BAD_PARAM, "SlidingWindowMathExpressionFilter: window_size must be odd and at least 1 (got %d)", p->window_size);
  }
  if (p->edge_handling < TE_EDGE_INSIDE || p->edge_handling > TE_EDGE_MEAN)
    return fail(TE_ERR_BAD_PARAM, "SlidingWindowMathExpressionFilter: edge_handling is one of TE_EDGE_INSIDE, TE_EDGE_CROP, TE_EDGE_EMPTY, TE_EDGE_MEAN (got %d)", p->edge_handling);
  return TE_OK;
}

int te_window_expr_check(const char* text, int in_layer, te_expr_info* info) {
  if (!text) return fail(TE_ERR_INVALID_ARG, "te_window_expr_check: NULL");
  expr::Program p;
  if (const int rc = compile("te_window_expr_check", text, in_layer, &p)) return rc;
  if (info) fill_expr_info(p, info);
  return TE_OK;
}

int te_run_window_expression(te_ctx* c, const te_window_expr_params* p, const char* text, int in_layer, int out_layer, int map0, int nmaps) {
  if (!c || !p || !text) return fail(TE_ERR_INVALID_ARG, "te_run_window_expression: NULL");
  if (const int rc = te_window_expr_params_validate(p)) return rc;
  Call call{};
  if (const int rc = compile("te_run_window_expression", text, in_layer, &call.prog, c)) return rc;
  TraceRange tr("te_run_window_expression");
  CtxLock lk(c, /*beside_prefetch*/ true, bit(in_layer) | bit(out_layer));
  if (c->have_geo) HIP_TRY(hipSetDevice(c->device));
  if (const int rc = prepare("te_run_window_expression", c, p, in_layer, out_layer, map0, nmaps, &call)) return rc;
  c->window_counts_valid = false;
  HIP_TRY(hipMemsetAsync(call.a.counts, 0, 2 * sizeof(unsigned long long), c->stream));
  HIP_TRY(wexpr::launch(call.prog, call.a, call.plan, c->stream));
  c->window_counts_valid = true;
  return note_layer_written(c, out_layer);
}

int te_run_window_expression_region(te_ctx* c, const te_window_expr_params* p, const char* text, int in_layer, int out_layer, int map, int row0, int col0, int h,
                                    int w, int out_rect[4]) {
  const char* const who = "te_run_window_expression_region";
  if (!c || !p || !text || !out_rect) return fail(TE_ERR_INVALID_ARG, "%s: NULL", who);
  if (const int rc = te_window_expr_params_validate(p)) return rc;
  Call call{};
  if (const int rc = compile(who, text, in_layer, &call.prog, c)) return rc;
  TraceRange tr(who);
  CtxLock lk(c, /*beside_prefetch*/ true, bit(in_layer) | bit(out_layer));
  if (c->have_geo) HIP_TRY(hipSetDevice(c->device));
  // (the window before the layers: region_filter_layers marks out_layer as touched once its own checks have passed)
  int win = 0;
  if (c->have_geo)
    if (const char* why = wexpr::window_from_params(p->window_size, p->use_window_length, p->window_length, c->geo.res, &win))
      return fail(TE_ERR_BAD_PARAM, "%s: %s", who, why);
  if (c->have_geo && !wexpr::plan(c->geo.rows, c->geo.cols, win, call.prog.n_red, call.prog.n_outer, c->opt_window_expr_route).fits)
    return fail(TE_ERR_UNSUPPORTED, "%s: a map of %d x %d cells with a window of %d is more than the kernel indexes", who, c->geo.rows, c->geo.cols, win);
  const float* in = nullptr;
  float* out = nullptr;
  if (const int rc = region_filter_layers(who, c, in_layer, out_layer, map, row0, col0, h, w, &in, &out)) return rc;
  const region::Rect dirty = {row0, col0, row0 + h, col0 + w};
  const wexpr::RegionPlan plan = wexpr::region_plan(c->geo.rows, c->geo.cols, win, call.prog.n_red, call.prog.n_outer, c->opt_window_expr_route, dirty);
  HIP_TRY(c->cmem.window_counts.once(2 * sizeof(unsigned long long)));
  call.plan = plan.k;
  fill_args(c, p, in, out, 1, &call.a);
  c->window_counts_valid = false;
  HIP_TRY(hipMemsetAsync(call.a.counts, 0, 2 * sizeof(unsigned long long), c->stream));
  HIP_TRY(wexpr::launch(call.prog, call.a, call.plan, c->stream));
  c->window_counts_valid = true;
  write_rect(plan.out, out_rect);
  note_region_written(c, out_layer);
  return TE_OK;
}

int te_window_expression_stats(te_ctx* c, uint64_t counts[2]) {
  if (!c || !counts) return fail(TE_ERR_INVALID_ARG, "te_window_expression_stats: NULL");
  CtxLock lk(c);
  if (!c->window_counts_valid || !c->cmem.window_counts.p)
    return fail(TE_ERR_NOT_READY, "te_window_expression_stats: no te_run_window_expression has run on this context");
  return read_block_counts(c, c->cmem.window_counts, counts);
}

int te_time_window_expression_samples(te_ctx* c, const te_window_expr_params* p, const char* text, int in_layer, int out_layer, int warmup, int iters, float* ms) {
  if (!c || !ms || iters <= 0 || warmup < 0) return fail(TE_ERR_INVALID_ARG, "te_time_window_expression_samples: bad argument");
  if (in_layer == out_layer) return fail(TE_ERR_INVALID_ARG, "te_time_window_expression_samples: the input layer must survive the repeats (in_layer == out_layer)");
  if (!layer_call::known(layer_call::Facts(), in_layer))  // (a reference layer: the text is compiled without the user names)
    return refused("te_time_window_expression_samples", c, {TE_ERR_INVALID_ARG, layer_call::kBadInput, in_layer, false});
  const bool copy = !p || !text;  // the floor: a device copy of the layer
  te_window_expr_params q;
  te_window_expr_params_default(&q);
  Call call{};
  if (!copy) {
    if (const int rc = te_window_expr_params_validate(p)) return rc;
    q = *p;
  }
  if (const int rc = compile("te_time_window_expression_samples", copy ? "0" : text, in_layer, &call.prog)) return rc;
  CtxLock lk(c);
  if (c->have_geo) HIP_TRY(hipSetDevice(c->device));
  if (const int rc = prepare("te_time_window_expression_samples", c, &q, in_layer, out_layer, 0, c->have_geo ? c->geo.batch : 1, &call)) return rc;
  const size_t bytes = (size_t)c->geo.rows * c->geo.cols * (size_t)c->geo.batch * sizeof(float);
  c->window_counts_valid = false;
  const auto clear = [&]() -> int {
    HIP_TRY(hipMemsetAsync(call.a.counts, 0, 2 * sizeof(unsigned long long), c->stream));
    return TE_OK;
  };
  const auto body = [&]() -> int {
    if (!copy)
      HIP_TRY(wexpr::launch(call.prog, call.a, call.plan, c->stream));
    else
      HIP_TRY(hipMemcpyAsync(call.a.out, call.a.in, bytes, hipMemcpyDeviceToDevice, c->stream));
    return TE_OK;
  };
  if (const int rc = time_samples(c, /*locked*/ true, warmup, iters, ms, clear, body)) return rc;
  c->window_counts_valid = !copy;
  // out_layer now holds the result (or the copy): the facts of an upload of those values
  return note_layer_written(c, out_layer);
}

}  // extern "C"
