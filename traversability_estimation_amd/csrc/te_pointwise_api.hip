// te_pointwise_api.hip -- C-ABI of the two point-wise filters of a grid_map chain: te_run_threshold(_region) (ThresholdFilter;
// kernels: te_pointwise.hip) and te_copy_layer (DuplicationFilter, a copy on the device) (include/travgpu.h).  The context: te_ctx.h.
#include "te_ctx.h"
#include "te_pointwise_launch.h"

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
  CallWhere at;
  at.map0 = map0, at.nmaps = nmaps;
  if (const int rc = refused(who, c, layer_call::check_update(facts_of(c), layer, map0, nmaps), at)) return rc;
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
  CallWhere at;
  at.map0 = map, at.row0 = row0, at.col0 = col0, at.h = h, at.w = w;
  if (const int rc = refused(who, c, layer_call::check_update_region(facts_of(c), layer, map, row0, col0, h, w), at)) return rc;
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
  CallWhere at;
  at.map0 = map0, at.nmaps = nmaps;
  const layer_call::Verdict v = layer_call::check(facts_of(c), src, dst, map0, nmaps, 0);
  if (const int rc = refused(who, c, v, at)) return rc;
  if (v.in_place) return TE_OK;
  HIP_TRY(hipSetDevice(c->device));
  if (dst != TE_LAYER_ELEVATION)
    if (const int rc = ensure_input_layer(c, dst)) return rc;
  const size_t cells = (size_t)c->geo.rows * c->geo.cols;
  HIP_TRY(hipMemcpyAsync(layer_ptr(c, dst) + cells * (size_t)map0, layer_ptr(c, src) + cells * (size_t)map0, cells * (size_t)nmaps * sizeof(float), hipMemcpyDeviceToDevice,
                         c->stream));
  return note_layer_written(c, dst);
}

}  // extern "C"
