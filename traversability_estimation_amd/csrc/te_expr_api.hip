// te_expr_api.hip -- C-ABI of te_run_expression(_region) / te_expr_check, of te_run_layer_expression(_region) / te_expr_check_ctx
// (any output layer, the context's user layers as operands) and of te_run_layer_expression_thresholds(_region) (ThresholdFilters
// fused behind the expression) (include/travgpu.h): a general MathExpressionFilter expression over the resident layers.  The language and its compiler: te_expr.h; the kernels: te_expr.hip.  The context: te_ctx.h.
#include "te_ctx.h"
#include "te_expr_launch.h"
#include "te_region_plan.h"

using namespace te;
using namespace te::shim;

static_assert(expr::kOk == TE_OK && expr::kBadParam == TE_ERR_BAD_PARAM && expr::kUnsupported == TE_ERR_UNSUPPORTED, "te_expr.h restates te_status");

namespace {

// un: the user names that are operands beside the reference's, or NULL
int compile(const char* who, const char* text, expr::Program* p, const UserNames* un = nullptr) {
  char err[200];
  const int rc = expr::compile(text, p, err, sizeof(err), un ? un->v : nullptr, un ? un->n : 0);
  return rc == TE_OK ? TE_OK : fail(rc, "%s: %s", who, err);
}

// the thresholds of te_run_layer_expression_thresholds behind the main code of a compiled program
int append_thresholds(const char* who, expr::Program* p, int n, const te_threshold* t) {
  if (n < 0 || n > TE_MAX_FUSED_THRESHOLDS || (n > 0 && !t)) return fail(TE_ERR_INVALID_ARG, "%s: %d thresholds (0 .. %d)", who, n, TE_MAX_FUSED_THRESHOLDS);
  expr::Threshold th[TE_MAX_FUSED_THRESHOLDS];
  for (int k = 0; k < n; ++k) {
    if (t[k].mode != TE_THRESHOLD_LOWER && t[k].mode != TE_THRESHOLD_UPPER) return fail(TE_ERR_INVALID_ARG, "%s: threshold %d: bad mode %d", who, k, t[k].mode);
    if (t[k].threshold != t[k].threshold) return fail(TE_ERR_INVALID_ARG, "%s: threshold %d is NaN", who, k);
    th[k] = expr::Threshold{t[k].mode == TE_THRESHOLD_LOWER, (float)t[k].threshold, (float)t[k].set_to};
  }
  char err[200];
  const int rc = expr::append_thresholds(p, n, th, err, sizeof(err));
  return rc == TE_OK ? TE_OK : fail(rc, "%s: %s", who, err);
}

// the layers the program reads, as the launch takes them; caller holds the lock.  Every refusal comes before the first launch.
int make_args(const char* who, te_ctx* c, const expr::Program& p, expr::Args& a) {
  memset(&a, 0, sizeof(a));
  const layer_call::Facts f = facts_of(c);
  for (int k = 0; k < p.n_layers; ++k) {
    const int id = p.layer_id[k];
    if (const int rc = refused(who, c, layer_call::check_expression_operand(f, id))) return rc;
    a.in[k] = layer_ptr(c, id);
  }
  a.out = c->L.trav;
  a.cells = (size_t)c->geo.rows * c->geo.cols;
  a.total = a.cells * (size_t)c->geo.batch;
  return TE_OK;
}

int launch_locked(te_ctx* c, const expr::Program& p, const expr::Args& a) {
  void* scratch = nullptr;
  if (p.n_red > 0) {
    HIP_TRY(c->lmem.expr_scratch.reserve(expr::scratch_bytes(p, a.cells, (size_t)c->geo.batch), c->stream));
    scratch = c->lmem.expr_scratch.p;
  }
  HIP_TRY(expr::launch(p, a, (size_t)c->geo.batch, scratch, c->stream));
  return TE_OK;
}

}  // namespace

// The rectangle form, shared with te_run_chain_region_expression (te_shim.hip; declared in te_ctx.h)
namespace te {
namespace shim {

void fill_expr_info(const expr::Program& p, te_expr_info* info) {
  info->n_instructions = p.n_code;
  info->layer_mask = expr::layer_mask(p);
  info->n_reductions = p.n_red;
  info->stack_depth = p.stack_depth;
}

// compiles `text` and refuses what has no rectangle form; touches no context
int region_expression_program(const char* who, const char* text, expr::Program* p, const UserNames* un, int out_layer) {
  if (const int rc = compile(who, text, p, un)) return rc;
  if (p->n_red > 0)
    return fail(TE_ERR_UNSUPPORTED, "%s: the expression has a reduction over the whole map, which a changed cell carries to every cell: "
                                    "run te_run_expression", who);
  if (out_layer != TE_LAYER_TRAVERSABILITY && (expr::layer_mask(*p) & bit(out_layer)))
    return fail(TE_ERR_UNSUPPORTED, "%s: the expression reads the layer it writes: what the whole-map call would write now is not defined for a "
                                    "rectangle recomputed in place; run te_run_layer_expression", who);
  if (out_layer == TE_LAYER_TRAVERSABILITY && (expr::layer_mask(*p) & bit(TE_LAYER_TRAVERSABILITY)))
    return fail(TE_ERR_UNSUPPORTED, "%s: the expression reads the traversability layer it writes: what the whole-map call would write now is "
                                    "not defined for a rectangle recomputed in place; run te_run_expression", who);
  return TE_OK;
}

// the layers the program reads (TE_ERR_NOT_READY: one is missing); caller holds the lock; launches and changes nothing
int region_expression_args(const char* who, te_ctx* c, const expr::Program& p, expr::Args* a) {
  if (!c->have_geo) return fail(TE_ERR_NOT_READY, "%s: geometry not set", who);
  return make_args(who, c, p, *a);
}

// the kernel on the rectangle (checked by the caller), then the facts of te_upload_layer_tile(out_layer)
int region_expression_launch(const char* who, te_ctx* c, const expr::Program& p, const expr::Args& a, int map, int row0, int col0, int h, int w, int out_layer) {
  HIP_TRY(hipSetDevice(c->device));
  const hipError_t e = expr::launch_rect(p, a, c->geo.rows, c->geo.cols, map, row0, col0, h, w, c->stream);
  if (e == hipErrorInvalidValue) {
    (void)hipGetLastError();
    return fail(TE_ERR_INVALID_ARG, "%s: rectangle (%d,%d)+(%d,%d) of map %d outside %dx%d", who, row0, col0, h, w, map, c->geo.rows, c->geo.cols);
  }
  HIP_TRY(e);
  if (out_layer == TE_LAYER_TRAVERSABILITY)
    c->st.expression_wrote_traversability_region();
  else
    note_region_written(c, out_layer);
  return TE_OK;
}

}  // namespace shim
}  // namespace te

extern "C" {

int te_expr_check(const char* text, te_expr_info* info) {
  if (!text) return fail(TE_ERR_INVALID_ARG, "te_expr_check: NULL");
  expr::Program p;
  if (const int rc = compile("te_expr_check", text, &p)) return rc;
  if (info) fill_expr_info(p, info);
  return TE_OK;
}

int te_run_expression(te_ctx* c, const char* text, int out_layer) {
  if (!c || !text) return fail(TE_ERR_INVALID_ARG, "te_run_expression: NULL");
  if (out_layer != TE_LAYER_TRAVERSABILITY)
    return fail(TE_ERR_INVALID_ARG, "te_run_expression: the output layer must be traversability (TE_LAYER_TRAVERSABILITY), got %d", out_layer);
  expr::Program p;
  if (const int rc = compile("te_run_expression", text, &p)) return rc;
  TraceRange tr("te_run_expression");
  CtxLock lk(c, /*beside_prefetch*/ true, expr::layer_mask(p) | bit(TE_LAYER_TRAVERSABILITY));
  if (!c->have_geo) return fail(TE_ERR_NOT_READY, "te_run_expression: geometry not set");
  expr::Args a;
  if (const int rc = make_args("te_run_expression", c, p, a)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if (const int rc = launch_locked(c, p, a)) return rc;
  // as te_upload_layer(TE_LAYER_TRAVERSABILITY) leaves it: the values are not bounded by the weights
  c->st.expression_wrote_traversability();
  return TE_OK;
}

int te_run_expression_region(te_ctx* c, const char* text, int out_layer, int map, int row0, int col0, int h, int w) {
  const char* const who = "te_run_expression_region";
  if (!c || !text) return fail(TE_ERR_INVALID_ARG, "%s: NULL", who);
  if (out_layer != TE_LAYER_TRAVERSABILITY)
    return fail(TE_ERR_INVALID_ARG, "%s: the output layer must be traversability (TE_LAYER_TRAVERSABILITY), got %d", who, out_layer);
  expr::Program p;
  if (const int rc = region_expression_program(who, text, &p)) return rc;
  TraceRange tr(who);
  CtxLock lk(c, /*beside_prefetch*/ true, expr::layer_mask(p) | bit(TE_LAYER_TRAVERSABILITY));
  if (!c->have_geo) return fail(TE_ERR_NOT_READY, "%s: geometry not set", who);
  if (map < 0 || map >= c->geo.batch) return fail(TE_ERR_INVALID_ARG, "%s: map %d of batch %d", who, map, c->geo.batch);
  if (!region::valid_rect(c->geo.rows, c->geo.cols, row0, col0, h, w))
    return fail(TE_ERR_INVALID_ARG, "%s: rectangle (%d,%d)+(%d,%d) outside %dx%d", who, row0, col0, h, w, c->geo.rows, c->geo.cols);
  expr::Args a;
  if (const int rc = region_expression_args(who, c, p, &a)) return rc;
  return region_expression_launch(who, c, p, a, map, row0, col0, h, w);
}

int te_expr_check_ctx(te_ctx* c, const char* text, te_expr_info* info) {
  if (!c || !text) return fail(TE_ERR_INVALID_ARG, "te_expr_check_ctx: NULL");
  UserNames un;
  snapshot_user_names(c, &un);
  expr::Program p;
  if (const int rc = compile("te_expr_check_ctx", text, &p, &un)) return rc;
  if (info) fill_expr_info(p, info);
  return TE_OK;
}

namespace {

// out_layer before the context is looked at: an id that can be a layer at all
int possible_out_layer(const char* who, int out_layer) {
  if (out_layer >= 0 && out_layer < TE_LAYER_COUNT + TE_MAX_USER_LAYERS) return TE_OK;
  return refused(who, nullptr, {TE_ERR_INVALID_ARG, layer_call::kBadOutput, out_layer, false});
}

int run_layer_expression(const char* who, te_ctx* c, const char* text, int out_layer, int n, const te_threshold* t) {
  if (!c || !text) return fail(TE_ERR_INVALID_ARG, "%s: NULL", who);
  if (const int rc = possible_out_layer(who, out_layer)) return rc;
  UserNames un;
  snapshot_user_names(c, &un);
  expr::Program p;
  if (const int rc = compile(who, text, &p, &un)) return rc;
  if (const int rc = append_thresholds(who, &p, n, t)) return rc;
  TraceRange tr(who);
  CtxLock lk(c, /*beside_prefetch*/ true, expr::layer_mask(p) | bit(out_layer));
  if (!c->have_geo) return fail(TE_ERR_NOT_READY, "%s: geometry not set", who);
  if (const int rc = refused(who, c, layer_call::check_expression_output(facts_of(c), out_layer))) return rc;  // (allocates nothing)
  expr::Args a;
  if (const int rc = make_args(who, c, p, a)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if (out_layer != TE_LAYER_TRAVERSABILITY && out_layer != TE_LAYER_ELEVATION)
    if (const int rc = ensure_input_layer(c, out_layer)) return rc;  // (the memory of robot_slope or a user layer; as an upload)
  a.out = layer_ptr(c, out_layer);  // (in place: make_args has refused a text that reads a layer without memory)
  if (const int rc = launch_locked(c, p, a)) return rc;
  if (out_layer == TE_LAYER_TRAVERSABILITY) {
    c->st.expression_wrote_traversability();
    return TE_OK;
  }
  return note_layer_written(c, out_layer);  // as te_upload_layer(out_layer) leaves it
}

int run_layer_expression_region(const char* who, te_ctx* c, const char* text, int out_layer, int n, const te_threshold* t, int map, int row0, int col0, int h,
                                int w) {
  if (!c || !text) return fail(TE_ERR_INVALID_ARG, "%s: NULL", who);
  if (const int rc = possible_out_layer(who, out_layer)) return rc;
  UserNames un;
  snapshot_user_names(c, &un);
  expr::Program p;
  if (const int rc = region_expression_program(who, text, &p, &un, out_layer)) return rc;
  if (const int rc = append_thresholds(who, &p, n, t)) return rc;
  TraceRange tr(who);
  CtxLock lk(c, /*beside_prefetch*/ true, expr::layer_mask(p) | bit(out_layer));
  if (!c->have_geo) return fail(TE_ERR_NOT_READY, "%s: geometry not set", who);
  if (const int rc = refused(who, c, layer_call::check_expression_output(facts_of(c), out_layer))) return rc;  // (allocates nothing)
  if (map < 0 || map >= c->geo.batch) return fail(TE_ERR_INVALID_ARG, "%s: map %d of batch %d", who, map, c->geo.batch);
  if (!region::valid_rect(c->geo.rows, c->geo.cols, row0, col0, h, w))
    return fail(TE_ERR_INVALID_ARG, "%s: rectangle (%d,%d)+(%d,%d) outside %dx%d", who, row0, col0, h, w, c->geo.rows, c->geo.cols);
  expr::Args a;
  if (const int rc = region_expression_args(who, c, p, &a)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if (out_layer != TE_LAYER_TRAVERSABILITY && out_layer != TE_LAYER_ELEVATION)
    if (const int rc = ensure_input_layer(c, out_layer)) return rc;
  a.out = layer_ptr(c, out_layer);
  return region_expression_launch(who, c, p, a, map, row0, col0, h, w, out_layer);
}

}  // namespace

int te_run_layer_expression(te_ctx* c, const char* text, int out_layer) { return run_layer_expression("te_run_layer_expression", c, text, out_layer, 0, nullptr); }

int te_run_layer_expression_region(te_ctx* c, const char* text, int out_layer, int map, int row0, int col0, int h, int w) {
  return run_layer_expression_region("te_run_layer_expression_region", c, text, out_layer, 0, nullptr, map, row0, col0, h, w);
}

int te_run_layer_expression_thresholds(te_ctx* c, const char* text, int out_layer, int n, const te_threshold* t) {
  return run_layer_expression("te_run_layer_expression_thresholds", c, text, out_layer, n, t);
}

int te_run_layer_expression_thresholds_region(te_ctx* c, const char* text, int out_layer, int n, const te_threshold* t, int map, int row0, int col0, int h,
                                              int w) {
  return run_layer_expression_region("te_run_layer_expression_thresholds_region", c, text, out_layer, n, t, map, row0, col0, h, w);
}

int te_time_expression_samples(te_ctx* c, const char* text, int warmup, int iters, float* ms) {
  if (!c || !ms || iters <= 0 || warmup < 0) return fail(TE_ERR_INVALID_ARG, "te_time_expression_samples: bad argument");
  const auto body = [&]() -> int { return text ? te_run_expression(c, text, TE_LAYER_TRAVERSABILITY) : te_run_filter(c, TE_FILTER_COMBINE, 0); };
  return time_samples(c, /*locked*/ false, warmup, iters, ms, [] { return TE_OK; }, body);
}

}  // extern "C"
