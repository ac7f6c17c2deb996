// te_median_api.hip -- C-ABI of te_run_median_fill / te_download_fill_mask (include/travgpu.h: MedianFillFilter on the device).
// The plan: te_median_plan.h; the selection: te_median.h; the kernels: te_median.hip.  The context: te_ctx.h.
#include "te_ctx.h"
#include "te_median_launch.h"

using namespace te;
using namespace te::shim;

// shared with te_radius_api.hip (declared in te_ctx.h)
namespace te {
namespace shim {

int reserve_scratch(const char* who, DevBuf& b, size_t bytes, hipStream_t stream, const char* what) {
  const hipError_t e = b.reserve(bytes, stream);
  if (e != hipSuccess) return fail(TE_ERR_UNSUPPORTED, "%s: %s (%zu bytes) does not fit in device memory: %s", who, what, bytes, hipGetErrorString(e));
  return TE_OK;
}

// the context's facts about a layer a device filter (te_run_median_fill, te_run_radius_filter) has written: those of an upload of the same values (te_upload_elevation /
// te_upload_layer); caller holds the lock
int note_layer_written(te_ctx* c, int out_layer) {
  if (out_layer == TE_LAYER_ELEVATION) {
    c->st.elevation_replaced();
    // the pass of an elevation upload over the whole layer: invalid cells, their runs, the face flags (it waits for the fill)
    return count_invalid_elevation(c);
  }
  c->st.layer_written(out_layer, CtxState::kUploaded);
  return TE_OK;
}

// The checks of a region filter (te_run_median_fill_region, te_run_radius_filter_region, te_run_window_expression_region):
// te_layer_call.h, check_region.  On success *in / *out point at the cells of `map`.  Nothing is touched before every check
// has passed.
int region_filter_layers(const char* who, te_ctx* c, int in_layer, int out_layer, int map, int row0, int col0, int h, int w, const float** in, float** out) {
  CallWhere at;
  at.map0 = map, at.row0 = row0, at.col0 = col0, at.h = h, at.w = w;
  if (const int rc = refused(who, c, layer_call::check_region(facts_of(c), in_layer, out_layer, map, row0, col0, h, w), at)) return rc;
  if (const int rc = ensure_input_layer(c, out_layer)) return rc;  // (robot_slope exists from its first write on)
  const size_t cells = (size_t)c->geo.rows * c->geo.cols;
  *in = layer_ptr(c, in_layer) + cells * (size_t)map;
  *out = layer_ptr(c, out_layer) + cells * (size_t)map;
  return TE_OK;
}

// the context's facts after a region filter wrote `out_layer`: the elevation as te_upload_tile leaves it (the done-flags stay,
// counts and face flags are unknown: te_ctx_state.h, elevation_tile_written), any other layer as te_upload_layer
void note_region_written(te_ctx* c, int out_layer) {
  if (out_layer == TE_LAYER_ELEVATION)
    c->st.elevation_tile_written();
  else
    c->st.layer_written(out_layer, CtxState::kUploaded);
}

}  // namespace shim
}  // namespace te

namespace {

struct Call {
  median::Args a;
  median::Plan plan;
};

// the radii of the two windows in cells; r_exist -1: finite cells keep their value
void window_radii(const te_ctx* c, const te_median_fill_params* p, int* r_fill, int* r_exist) {
  const int rows = c->geo.rows, cols = c->geo.cols;
  *r_fill = median::radius_cells(p->fill_hole_radius, c->geo.res, rows, cols);
  *r_exist = -1;
  if (p->filter_existing_values) {
    *r_exist = median::radius_cells(p->existing_value_radius, c->geo.res, rows, cols);
    if (*r_exist == 0) *r_exist = -1;  // the median of a finite cell's window of one cell is the cell
  }
}

// checks, scratch and plan of one call; caller holds the lock and has made the device current.  With in_layer == out_layer
// the kernels read a copy of the input, queued here.
int prepare(const char* who, te_ctx* c, const te_median_fill_params* p, int in_layer, int out_layer, int map0, int nmaps, Call* call) {
  CallWhere at;
  at.map0 = map0, at.nmaps = nmaps;
  if (const int rc = refused(who, c, layer_call::check(facts_of(c), in_layer, out_layer, map0, nmaps, 0), at)) return rc;
  if (in_layer != out_layer)
    if (const int rc = ensure_input_layer(c, out_layer)) return rc;  // (robot_slope exists from its first write on)
  const float* const in = layer_ptr(c, in_layer);
  float* const out = layer_ptr(c, out_layer);

  const int rows = c->geo.rows, cols = c->geo.cols;
  const size_t cells = (size_t)rows * cols, total = cells * (size_t)nmaps;
  int r_fill = 0, r_exist = -1;
  window_radii(c, p, &r_fill, &r_exist);
  const median::Plan plan = median::plan(rows, cols, nmaps, std::max(r_fill, r_exist), c->opt_median_route);
  if (plan.route == median::kRouteAny && cells >= ((size_t)1 << 32))
    return fail(TE_ERR_UNSUPPORTED, "%s: a window radius of %d cells takes the general kernel, which lists cells in 32 bits: %zu cells per map are too many", who, plan.r, cells);

  te_ctx::LayerMem& m = c->lmem;
  const float* in_first = in + cells * map0;  // the first map of the call
  const size_t batch_cells = cells * (size_t)c->geo.batch;
  if (const int rc = reserve_scratch(who, m.median_mask, batch_cells, c->stream, "the fill mask")) return rc;
  if (const int rc = reserve_scratch(who, m.median_tmp, 2 * batch_cells, c->stream, "the scratch masks")) return rc;
  if (plan.route == median::kRouteAny)
    if (const int rc = reserve_scratch(who, m.median_any, (median::any_blocks(cells) + 1 + cells) * sizeof(unsigned), c->stream, "the list of cells")) return rc;
  if (in_layer == out_layer) {
    if (const int rc = reserve_scratch(who, m.median_copy, c->layer_elems * sizeof(float), c->stream, "the copy of the input layer")) return rc;
    HIP_TRY(hipMemcpyAsync(m.median_copy.p, in_first, total * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    in_first = m.median_copy.as<float>();
  }
  median::Args& a = call->a;
  a.in = in_first;
  a.out = out + cells * map0;
  a.mask = m.median_mask.as<uint8_t>() + cells * map0;
  a.tmp[0] = m.median_tmp.as<uint8_t>();
  a.tmp[1] = m.median_tmp.as<uint8_t>() + batch_cells;
  a.any_counts = m.median_any.as<unsigned>();
  a.any_list = a.any_counts ? a.any_counts + median::any_blocks(cells) + 1 : nullptr;
  a.rows = rows;
  a.cols = cols;
  a.nmaps = nmaps;
  a.r_fill = r_fill;
  a.r_exist = r_exist;
  a.iterations = p->num_erode_dilation_iterations;
  call->plan = plan;
  return TE_OK;
}

}  // namespace

extern "C" {

int te_median_fill_params_default(te_median_fill_params* p) {
  if (!p) return fail(TE_ERR_INVALID_ARG, "te_median_fill_params_default: NULL");
  memset(p, 0, sizeof(*p));
  p->size = (uint32_t)sizeof(te_median_fill_params);
  p->abi_version = TE_ABI_VERSION;
  // grid_map_filters MedianFillFilter::configure(), as remembered (travgpu.h)
  p->fill_hole_radius = 0.05;
  p->filter_existing_values = 0;
  p->existing_value_radius = 0.0;
  p->num_erode_dilation_iterations = 4;
  return TE_OK;
}

int te_median_fill_params_validate(const te_median_fill_params* p) {
  if (!p) return fail(TE_ERR_INVALID_ARG, "te_median_fill_params: NULL");
  if (p->size != sizeof(te_median_fill_params) || p->abi_version != TE_ABI_VERSION)
    return fail(TE_ERR_INVALID_ARG, "te_median_fill_params: size/abi mismatch (got %u/%u, want %zu/%d)", p->size, p->abi_version, sizeof(te_median_fill_params),
                TE_ABI_VERSION);
  if (!(p->fill_hole_radius >= 0.0) || !isfinite(p->fill_hole_radius)) return fail(TE_ERR_BAD_PARAM, "MedianFillFilter: fill_hole_radius must be finite and not negative");
  if (!(p->existing_value_radius >= 0.0) || !isfinite(p->existing_value_radius))
    return fail(TE_ERR_BAD_PARAM, "MedianFillFilter: existing_value_radius must be finite and not negative");
  if (p->num_erode_dilation_iterations < 0) return fail(TE_ERR_BAD_PARAM, "MedianFillFilter: num_erode_dilation_iterations must not be negative");
  return TE_OK;
}

int te_run_median_fill(te_ctx* c, const te_median_fill_params* p, int in_layer, int out_layer, int map0, int nmaps) {
  if (!c || !p) return fail(TE_ERR_INVALID_ARG, "te_run_median_fill: NULL");
  if (const int rc = te_median_fill_params_validate(p)) return rc;
  TraceRange tr("te_run_median_fill");
  CtxLock lk(c, /*beside_prefetch*/ true, bit(in_layer) | bit(out_layer));
  Call call{};
  if (c->have_geo) HIP_TRY(hipSetDevice(c->device));
  if (const int rc = prepare("te_run_median_fill", c, p, in_layer, out_layer, map0, nmaps, &call)) return rc;
  HIP_TRY(median::launch(call.a, call.plan, c->stream));
  if (c->fill_mask_valid.size() != (size_t)c->geo.batch) c->fill_mask_valid.assign((size_t)c->geo.batch, 0);
  for (int m = map0; m < map0 + nmaps; ++m) c->fill_mask_valid[(size_t)m] = 1;
  return note_layer_written(c, out_layer);
}

int te_run_median_fill_region(te_ctx* c, const te_median_fill_params* p, int in_layer, int out_layer, int map, int row0, int col0, int h, int w, int out_rect[4]) {
  const char* const who = "te_run_median_fill_region";
  if (!c || !p || !out_rect) return fail(TE_ERR_INVALID_ARG, "%s: NULL", who);
  if (const int rc = te_median_fill_params_validate(p)) return rc;
  TraceRange tr(who);
  CtxLock lk(c, /*beside_prefetch*/ true, bit(in_layer) | bit(out_layer));
  if (c->have_geo) HIP_TRY(hipSetDevice(c->device));
  const float* in = nullptr;
  float* out = nullptr;
  if (const int rc = region_filter_layers(who, c, in_layer, out_layer, map, row0, col0, h, w, &in, &out)) return rc;
  const int rows = c->geo.rows, cols = c->geo.cols;
  const size_t cells = (size_t)rows * cols, batch_cells = cells * (size_t)c->geo.batch;
  int r_fill = 0, r_exist = -1;
  window_radii(c, p, &r_fill, &r_exist);
  const region::Rect dirty = {row0, col0, row0 + h, col0 + w};
  const median::RegionPlan plan = median::region_plan(rows, cols, r_fill, r_exist, p->num_erode_dilation_iterations, c->opt_median_route, dirty);
  if (plan.k.route == median::kRouteAny && cells >= ((size_t)1 << 32))
    return fail(TE_ERR_UNSUPPORTED, "%s: a window radius of %d cells takes the general kernel, which lists cells in 32 bits: %zu cells per map are too many", who, plan.k.r, cells);
  // the stored mask and the scratch masks are addressed by map cell: the allocations of the whole-map call, made here if
  // none preceded (the mask then holds nothing to refresh: fill_mask_valid stays as it is); the list is sized by the region
  te_ctx::LayerMem& m = c->lmem;
  if (const int rc = reserve_scratch(who, m.median_mask, batch_cells, c->stream, "the fill mask")) return rc;
  if (const int rc = reserve_scratch(who, m.median_tmp, 2 * batch_cells, c->stream, "the scratch masks")) return rc;
  if (plan.k.route == median::kRouteAny)
    if (const int rc = reserve_scratch(who, m.median_any, (plan.any_blocks + 1 + region::cells(plan.out)) * sizeof(unsigned), c->stream, "the list of cells")) return rc;
  median::Args a{};
  a.in = in;
  a.out = out;
  a.mask = m.median_mask.as<uint8_t>() + cells * (size_t)map;
  a.tmp[0] = m.median_tmp.as<uint8_t>();
  a.tmp[1] = m.median_tmp.as<uint8_t>() + batch_cells;
  a.any_counts = m.median_any.as<unsigned>();
  a.any_list = a.any_counts ? a.any_counts + plan.any_blocks + 1 : nullptr;
  a.rows = rows;
  a.cols = cols;
  a.nmaps = 1;
  a.r_fill = r_fill;
  a.r_exist = r_exist;
  a.iterations = p->num_erode_dilation_iterations;
  HIP_TRY(median::launch_region(a, plan, c->stream));
  write_rect(plan.out, out_rect);
  note_region_written(c, out_layer);
  return TE_OK;
}

int te_download_fill_mask(te_ctx* c, int map, unsigned char* out, size_t bytes) {
  if (!c || !out) return fail(TE_ERR_INVALID_ARG, "te_download_fill_mask: NULL");
  CtxLock lk(c);
  if (!c->have_geo) return fail(TE_ERR_NOT_READY, "te_download_fill_mask: geometry not set");
  if (map < 0 || map >= c->geo.batch) return fail(TE_ERR_INVALID_ARG, "te_download_fill_mask: map %d of batch %d", map, c->geo.batch);
  if (c->fill_mask_valid.size() != (size_t)c->geo.batch || !c->fill_mask_valid[(size_t)map] || !c->lmem.median_mask.p)
    return fail(TE_ERR_NOT_READY, "te_download_fill_mask: no te_run_median_fill has covered map %d under this geometry", map);
  const size_t cells = (size_t)c->geo.rows * c->geo.cols;
  if (bytes != cells) return fail(TE_ERR_INVALID_ARG, "te_download_fill_mask: %zu bytes given, the mask is %zu", bytes, cells);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(out, c->lmem.median_mask.as<uint8_t>() + cells * (size_t)map, cells, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return TE_OK;
}

int te_time_median_fill_samples(te_ctx* c, const te_median_fill_params* p, int in_layer, int out_layer, int warmup, int iters, float* ms) {
  if (!c || !ms || iters <= 0 || warmup < 0) return fail(TE_ERR_INVALID_ARG, "te_time_median_fill_samples: bad argument");
  if (in_layer == out_layer) return fail(TE_ERR_INVALID_ARG, "te_time_median_fill_samples: the input layer must survive the repeats (in_layer == out_layer)");
  te_median_fill_params q;
  te_median_fill_params_default(&q);
  if (p) {
    if (const int rc = te_median_fill_params_validate(p)) return rc;
    q = *p;
  }
  CtxLock lk(c);
  if (c->have_geo) HIP_TRY(hipSetDevice(c->device));
  Call call{};
  if (const int rc = prepare("te_time_median_fill_samples", c, &q, in_layer, out_layer, 0, c->have_geo ? c->geo.batch : 1, &call)) return rc;
  const size_t bytes = (size_t)c->geo.rows * c->geo.cols * (size_t)c->geo.batch * sizeof(float);
  const auto body = [&]() -> int {
    if (p)
      HIP_TRY(median::launch(call.a, call.plan, c->stream));
    else
      HIP_TRY(hipMemcpyAsync(call.a.out, call.a.in, bytes, hipMemcpyDeviceToDevice, c->stream));
    return TE_OK;
  };
  if (const int rc = time_samples(c, /*locked*/ true, warmup, iters, ms, [] { return TE_OK; }, body)) return rc;
  // out_layer now holds the fill (or the copy): the facts of an upload of those values
  if (p) {
    c->fill_mask_valid.assign((size_t)c->geo.batch, 1);
  }
  return note_layer_written(c, out_layer);
}

}  // extern "C"
