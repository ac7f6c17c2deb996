// te_pointwise_api.hip -- C-ABI of the two point-wise filters of a grid_map chain: te_run_threshold(_region) (ThresholdFilter;
// kernels: te_pointwise.hip) and te_copy_layer (DuplicationFilter, a copy on the device) (include/travgpu.h).  The context: te_ctx.h.
#include "te_ctx.h"
#include "te_pointwise_launch.h"
#include "te_region_plan.h"

using namespace te;
using namespace te::shim;

namespace {

int check_threshold(const char* who, int mode, double threshold) {
  if (mode != TE_THRESHOLD_LOWER && mode != TE_THRESHOLD_UPPER) return fail(TE_ERR_INVALID_ARG, "%s: bad mode %d (TE_THRESHOLD_LOWER, TE_THRESHOLD_UPPER)", who, mode);
  if (threshold != threshold) return fail(TE_ERR_INVALID_ARG, "%s: the threshold is NaN", who);
  return TE_OK;
}

}  // namespace

extern "C" {

int te_run_threshold(te_ctx* c, int layer, int mode, double threshold, double set_to, int map0, int nmaps) {
  const char* const who = "te_run_threshold";
  if (!c) return fail(TE_ERR_INVALID_ARG, "%s: NULL ctx", who);
  if (const int rc = check_threshold(who, mode, threshold)) return rc;
  TraceRange tr(who);
  CtxLock lk(c, /*beside_prefetch*/ true, bit(layer));
  if (!c->have_geo) return fail(TE_ERR_NOT_READY, "%s: geometry not set", who);
  if (map0 < 0 || nmaps <= 0 || map0 > c->geo.batch - nmaps) return fail(TE_ERR_INVALID_ARG, "%s: maps [%d,%d) of batch %d", who, map0, map0 + nmaps, c->geo.batch);
  const float* in = nullptr;
  if (const int rc = filter_input_layer(who, c, layer, &in)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const size_t cells = (size_t)c->geo.rows * c->geo.cols;
  if (layer != TE_LAYER_ELEVATION) c->st.layer_touched(layer);  // (as an upload passes ensure_input_layer)
  HIP_TRY(pointwise::launch_threshold(layer_ptr(c, layer) + cells * (size_t)map0, cells * (size_t)nmaps, mode == TE_THRESHOLD_LOWER, (float)threshold,
                                      (float)set_to, c->stream));
  return note_layer_written(c, layer);
}

int te_run_threshold_region(te_ctx* c, int layer, int mode, double threshold, double set_to, int map, int row0, int col0, int h, int w) {
  const char* const who = "te_run_threshold_region";
  if (!c) return fail(TE_ERR_INVALID_ARG, "%s: NULL ctx", who);
  if (const int rc = check_threshold(who, mode, threshold)) return rc;
  TraceRange tr(who);
  CtxLock lk(c, /*beside_prefetch*/ true, bit(layer));
  if (!c->have_geo) return fail(TE_ERR_NOT_READY, "%s: geometry not set", who);
  if (map < 0 || map >= c->geo.batch) return fail(TE_ERR_INVALID_ARG, "%s: map %d of batch %d", who, map, c->geo.batch);
  const float* in = nullptr;
  if (const int rc = filter_input_layer(who, c, layer, &in)) return rc;
  if (!region::valid_rect(c->geo.rows, c->geo.cols, row0, col0, h, w))
    return fail(TE_ERR_INVALID_ARG, "%s: rectangle (%d,%d)+(%d,%d) outside %dx%d", who, row0, col0, h, w, c->geo.rows, c->geo.cols);
  HIP_TRY(hipSetDevice(c->device));
  const size_t cells = (size_t)c->geo.rows * c->geo.cols;
  if (layer != TE_LAYER_ELEVATION) c->st.layer_touched(layer);
  HIP_TRY(pointwise::launch_threshold_rect(layer_ptr(c, layer) + cells * (size_t)map, c->geo.rows, c->geo.cols, row0, col0, h, w, mode == TE_THRESHOLD_LOWER,
                                           (float)threshold, (float)set_to, c->stream));
  note_region_written(c, layer);
  return TE_OK;
}

int te_copy_layer(te_ctx* c, int src, int dst, int map0, int nmaps) {
  const char* const who = "te_copy_layer";
  if (!c) return fail(TE_ERR_INVALID_ARG, "%s: NULL ctx", who);
  TraceRange tr(who);
  CtxLock lk(c, /*beside_prefetch*/ true, bit(src) | bit(dst));
  if (!c->have_geo) return fail(TE_ERR_NOT_READY, "%s: geometry not set", who);
  if (!layer_known(c, dst)) return fail(TE_ERR_INVALID_ARG, "%s: bad output layer %d", who, dst);
  if (map0 < 0 || nmaps <= 0 || map0 > c->geo.batch - nmaps) return fail(TE_ERR_INVALID_ARG, "%s: maps [%d,%d) of batch %d", who, map0, map0 + nmaps, c->geo.batch);
  const float* in = nullptr;
  if (const int rc = filter_input_layer(who, c, src, &in)) return rc;
  if (!layer_on_demand(c, dst) && !layer_ptr(c, dst)) return fail(TE_ERR_INVALID_ARG, "%s: the output layer %d has no memory yet", who, dst);
  if (src == dst) return TE_OK;
  HIP_TRY(hipSetDevice(c->device));
  if (dst != TE_LAYER_ELEVATION)
    if (const int rc = ensure_input_layer(c, dst)) return rc;
  const size_t cells = (size_t)c->geo.rows * c->geo.cols;
  HIP_TRY(hipMemcpyAsync(layer_ptr(c, dst) + cells * (size_t)map0, in + cells * (size_t)map0, cells * (size_t)nmaps * sizeof(float), hipMemcpyDeviceToDevice,
                         c->stream));
  return note_layer_written(c, dst);
}

}  // extern "C"
