// te_expr_api.hip -- C-ABI of te_run_expression(_region) / te_expr_check (include/travgpu.h): a general MathExpressionFilter expression
// over the resident layers.  The language and its compiler: te_expr.h; the kernels: te_expr.hip.  The context: te_ctx.h.
#include "te_ctx.h"
#include "te_expr_launch.h"
#include "te_region_plan.h"

using namespace te;
using namespace te::shim;

static_assert(expr::kOk == TE_OK && expr::kBadParam == TE_ERR_BAD_PARAM && expr::kUnsupported == TE_ERR_UNSUPPORTED, "te_expr.h restates te_status");

namespace {

int compile(const char* who, const char* text, expr::Program* p) {
  char err[200];
  const int rc = expr::compile(text, p, err, sizeof(err));
  return rc == TE_OK ? TE_OK : fail(rc, "%s: %s", who, err);
}

// the layers the program reads, as the launch takes them; caller holds the lock.  Every refusal comes before the first launch.
int make_args(const char* who, te_ctx* c, const expr::Program& p, expr::Args& a) {
  constexpr unsigned optional = bit(TE_LAYER_NORMAL_X) | bit(TE_LAYER_NORMAL_Y) | bit(TE_LAYER_NORMAL_Z) | bit(TE_LAYER_SLOPE_FOOTPRINT) |
                                bit(TE_LAYER_STEP_FOOTPRINT) | bit(TE_LAYER_ROUGHNESS_FOOTPRINT);
  memset(&a, 0, sizeof(a));
  for (int k = 0; k < p.n_layers; ++k) {
    const int id = p.layer_id[k];
    const float* ptr = layer_ptr(c, id);
    const bool absent = !ptr || (bit(id) & optional & ~c->st.layers_written()) || (id == TE_LAYER_ROBOT_SLOPE && !c->st.have_robot_slope());
    if (absent) {
      int n = 0;
      const expr::LayerName* names = expr::layer_names(&n);
      return fail(TE_ERR_NOT_READY, "%s: the layer %s does not exist yet", who, names[id].name);
    }
    a.in[k] = ptr;
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

// compiles `text` and refuses what has no rectangle form; touches no context
int region_expression_program(const char* who, const char* text, expr::Program* p) {
  if (const int rc = compile(who, text, p)) return rc;
  if (p->n_red > 0)
    return fail(TE_ERR_UNSUPPORTED, "%s: the expression has a reduction over the whole map, which a changed cell carries to every cell: "
                                    "run te_run_expression", who);
  if (expr::layer_mask(*p) & bit(TE_LAYER_TRAVERSABILITY))
    return fail(TE_ERR_UNSUPPORTED, "%s: the expression reads the traversability layer it writes: what the whole-map call would write now is "
                                    "not defined for a rectangle recomputed in place; run te_run_expression", who);
  return TE_OK;
}

// the layers the program reads (TE_ERR_NOT_READY: one is missing); caller holds the lock; launches and changes nothing
int region_expression_args(const char* who, te_ctx* c, const expr::Program& p, expr::Args* a) {
  if (!c->have_geo) return fail(TE_ERR_NOT_READY, "%s: geometry not set", who);
  return make_args(who, c, p, *a);
}

// the kernel on the rectangle (checked by the caller), then the facts of te_upload_layer_tile(TE_LAYER_TRAVERSABILITY)
int region_expression_launch(const char* who, te_ctx* c, const expr::Program& p, const expr::Args& a, int map, int row0, int col0, int h, int w) {
  HIP_TRY(hipSetDevice(c->device));
  const hipError_t e = expr::launch_rect(p, a, c->geo.rows, c->geo.cols, map, row0, col0, h, w, c->stream);
  if (e == hipErrorInvalidValue) {
    (void)hipGetLastError();
    return fail(TE_ERR_INVALID_ARG, "%s: rectangle (%d,%d)+(%d,%d) of map %d outside %dx%d", who, row0, col0, h, w, map, c->geo.rows, c->geo.cols);
  }
  HIP_TRY(e);
  c->st.expression_wrote_traversability_region();
  return TE_OK;
}

}  // namespace shim
}  // namespace te

extern "C" {

int te_expr_check(const char* text, te_expr_info* info) {
  if (!text) return fail(TE_ERR_INVALID_ARG, "te_expr_check: NULL");
  expr::Program p;
  if (const int rc = compile("te_expr_check", text, &p)) return rc;
  if (info) {
    info->n_instructions = p.n_code;
    info->layer_mask = expr::layer_mask(p);
    info->n_reductions = p.n_red;
    info->stack_depth = p.stack_depth;
  }
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

int te_time_expression_samples(te_ctx* c, const char* text, int warmup, int iters, float* ms) {
  if (!c || !ms || iters <= 0 || warmup < 0) return fail(TE_ERR_INVALID_ARG, "te_time_expression_samples: bad argument");
  for (int k = -warmup; k < iters; ++k) {
    {
      CtxLock lk(c);
      HIP_TRY(hipSetDevice(c->device));
      HIP_TRY(hipEventRecord(c->ev0, c->stream));
    }
    if (const int rc = text ? te_run_expression(c, text, TE_LAYER_TRAVERSABILITY) : te_run_filter(c, TE_FILTER_COMBINE, 0)) return rc;
    CtxLock lk(c);
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev1));
    float t = 0.0f;
    HIP_TRY(hipEventElapsedTime(&t, c->ev0, c->ev1));
    if (k >= 0) ms[k] = t;
  }
  return TE_OK;
}

}  // extern "C"
