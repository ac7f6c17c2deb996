// te_paths_api.hip -- C-ABI of libtravgpu.so, SURVEY.md 8(f) N2 / N3: batched checkFootprintPath (circular and polygonal,
// TraversabilityMap.cpp:320-645), checkInclination (:748-762), the polygon footprint layers (:239-305).  Kernels:
// te_paths.hip, te_polygon.hip.  The context and the helpers shared with the other parts: te_ctx.h.
#include "te_ctx.h"
#include "te_fp_table.h"
#include "te_path_visit.h"

using namespace te;
using namespace te::shim;

namespace {
// The spiral table of circle(radius + offset) on the device, from the context's cache or built now (te_fp_table.h: the
// table of the footprint pass at any reach).  A request with more classes than the cache holds keeps the rest in `temps`
// for the call.  first_clock: pd_clock when the call began (entries used since then serve this call and stay).
int path_disc_table(te_ctx* c, double radius, double offset, unsigned long long first_clock, std::vector<DevBuf>& temps,
                    PathDiscClass* out) {
  const Geo& g = c->geo;
  out->rmin = radius;
  out->rmax = radius + offset;
  out->r2 = out->rmax * out->rmax;
  out->pad = 0;
  te_ctx::PdTable* victim = nullptr;
  for (te_ctx::PdTable& t : c->lmem.pd_tables) {
    if (t.dev.p && t.radius == radius && t.offset == offset && t.res == g.res && t.rows == g.rows && t.cols == g.cols) {
      t.used = ++c->pd_clock;
      out->spiral = t.dev.as<const int4>();
      out->n_spiral = t.n_spiral;
      return TE_OK;
    }
    if ((!t.dev.p || t.used <= first_clock) && (!victim || (victim->dev.p && (!t.dev.p || t.used < victim->used)))) victim = &t;
  }
  FpTable tab;
  build_fp_table(out->rmax, g.res, g.rows, g.cols, &tab);
  const size_t bytes = tab.spiral.size() * sizeof(FpEntry);
  if (tab.spiral.size() > (size_t)0x7fffffff) return fail(TE_ERR_UNSUPPORTED, "te_check_footprint_paths_radius: a spiral of %zu entries", tab.spiral.size());
  DevBuf dev;
  hipError_t e = dev.once(bytes);
  if (e == hipSuccess) e = hipMemcpyAsync(dev.p, tab.spiral.data(), bytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // (tab goes out of scope; and the stream has drained before a victim's table is freed)
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(TE_ERR_HIP, "te_check_footprint_paths_radius: the spiral table of radius %g m (%zu bytes): %s", radius, bytes, hipGetErrorString(e));
  }
  out->spiral = dev.as<const int4>();
  out->n_spiral = (int)tab.spiral.size();
  if (victim) {
    victim->radius = radius;
    victim->offset = offset;
    victim->res = g.res;
    victim->rows = g.rows;
    victim->cols = g.cols;
    victim->dev = std::move(dev);
    victim->n_spiral = out->n_spiral;
    victim->used = ++c->pd_clock;
  } else {
    temps.push_back(std::move(dev));
  }
  return TE_OK;
}

// The untraversable mask (Layers::untrav), built on the first call after the scores (or one of the three parameters it
// reads) changed: every entry point whose kernels read the mask calls this before it launches one.  Queued on the
// context's stream, c->mu held.
hipError_t ensure_mask(te_ctx* c) {
  if (c->st.mask_done()) return hipSuccess;
  const hipError_t e = launch_footprint_mask(c->geo, c->fp, c->L, usable_face_flags(c), c->st.combine_deferred() ? &c->cp : nullptr, c->stream);
  if (e == hipSuccess) c->st.mask_built();
  return e;
}
}  // namespace

extern "C" {

int te_check_footprint_paths_radius(te_ctx* c, int map, int n_paths, const int* pose_offset, const double* pose_xy, const double* radius,
                                    double offset, unsigned char* is_safe, double* traversability, int* status,
                                    te_path_check_stats* stats) {
  if (!c || n_paths < 0 || (n_paths > 0 && (!pose_offset || !pose_xy || !radius || !is_safe || !traversability || !status)))
    return fail(TE_ERR_INVALID_ARG, "te_check_footprint_paths_radius: NULL argument");
  if (!isfinite(offset) || offset < 0.0) return fail(TE_ERR_INVALID_ARG, "te_check_footprint_paths_radius: offset %g", offset);
  for (int k = 0; k < n_paths; ++k)
    if (!isfinite(radius[k]) || radius[k] < 0.0)
      return fail(TE_ERR_INVALID_ARG, "te_check_footprint_paths_radius: radius[%d] = %g (a footprint radius is finite and not negative)", k, radius[k]);
  CtxLock lk(c);
  if (!c->have_geo || !c->st.chain_done() || !c->tables_ready)
    return fail(TE_ERR_NOT_READY, "te_check_footprint_paths_radius: run the filter chain first (it produces the layers the discs read)");
  if (map < 0 || map >= c->geo.batch) return fail(TE_ERR_INVALID_ARG, "te_check_footprint_paths_radius: map %d of %d", map, c->geo.batch);
  if (c->check_inclination && !c->st.have_robot_slope())
    return fail(TE_ERR_NOT_READY, "te_check_footprint_paths_radius: check_robot_inclination is set but the layer robot_slope was never uploaded");
  if (stats) stats->n_visits = stats->n_discs = stats->n_radius_classes = 0;
  if (n_paths == 0) return TE_OK;
  const int n_poses = pose_offset[n_paths];
  if (pose_offset[0] != 0 || n_poses < 0) return fail(TE_ERR_INVALID_ARG, "te_check_footprint_paths_radius: bad pose offsets");
  for (int k = 0; k < n_paths; ++k)
    if (pose_offset[k + 1] < pose_offset[k]) return fail(TE_ERR_INVALID_ARG, "te_check_footprint_paths_radius: bad pose offsets");
  // (the mask kernel takes the discs of its three checks from the footprint tables; they do not depend on fp_radius)
  if (!c->fp_tables_ready) return fail(c->fp_tables_rc ? c->fp_tables_rc : TE_ERR_NOT_READY, "%s", c->fp_tables_err);
  const Geo& g = c->geo;
  // the plan (te_path_visit.h): radius classes, and the number of visits, which sizes the memo
  std::vector<double> uniq;
  std::vector<int> cls;
  pv::class_radii(n_paths, radius, &uniq, &cls);
  if (uniq.size() > (size_t)pv::kMaxClasses)
    return fail(TE_ERR_UNSUPPORTED, "te_check_footprint_paths_radius: %zu distinct radii in one call (at most %d)", uniq.size(), pv::kMaxClasses);
  const pv::Geom hg = {g.rows, g.cols, g.res, g.len_x, g.len_y, g.pos_x, g.pos_y};
  unsigned long long n_visits = 0;
  for (int k = 0; k < n_paths; ++k)
    n_visits += (unsigned long long)pv::count_path_visits(hg, pose_offset[k + 1] - pose_offset[k], pose_xy + 2 * (size_t)pose_offset[k]);
  const uint64_t entries = pv::table_entries(n_visits);
  if (entries > ((uint64_t)1 << 31)) return fail(TE_ERR_UNSUPPORTED, "te_check_footprint_paths_radius: %llu centres in one call", n_visits);
  HIP_TRY(hipSetDevice(c->device));
  const unsigned long long first_clock = c->pd_clock;
  std::vector<PathDiscClass> classes(uniq.size());
  std::vector<DevBuf> temps;  // the tables of this call alone: freed when it returns, behind its stream synchronize
  for (size_t q = 0; q < uniq.size(); ++q)
    if (const int rc = path_disc_table(c, uniq[q], offset, first_clock, temps, &classes[q])) return rc;
  // one scratch buffer: the staged request and its results, the class array, the memo (keys, values, work list, counters)
  const size_t list_cap = n_visits > 0 ? (size_t)n_visits : 1;
  Carve cv;
  const auto p_keys = cv.add<uint64_t>((size_t)entries);
  const auto p_xy = cv.add<double>((size_t)2 * (n_poses > 0 ? n_poses : 1));
  const auto p_trav = cv.add<double>(n_paths);
  const auto p_classes = cv.add<PathDiscClass>(classes.size());
  const auto p_off = cv.add<int>((size_t)n_paths + 1);
  const auto p_cls = cv.add<int>(n_paths);
  const auto p_st = cv.add<int>(n_paths);
  const auto p_vals = cv.add<float>((size_t)entries);
  const auto p_list = cv.add<unsigned>(list_cap);
  const auto p_cnt = cv.add<unsigned>(kPdCounters);
  const auto p_safe = cv.add<unsigned char>(n_paths);
  DevBuf& scratch = c->lmem.pd_scratch;
  if (const hipError_t e = scratch.reserve(cv.total, c->stream))
    return fail(TE_ERR_HIP, "te_check_footprint_paths_radius: hipMalloc(%zu bytes) for %llu centres: %s", cv.total, n_visits, hipGetErrorString(e));
  PathDiscScratch s;
  s.keys = p_keys.in(scratch);
  double* d_xy = p_xy.in(scratch);
  double* d_trav = p_trav.in(scratch);
  PathDiscClass* d_classes = p_classes.in(scratch);
  int* d_off = p_off.in(scratch);
  int* d_cls = p_cls.in(scratch);
  int* d_st = p_st.in(scratch);
  s.vals = p_vals.in(scratch);
  s.list = p_list.in(scratch);
  s.counters = p_cnt.in(scratch);
  unsigned char* d_safe = p_safe.in(scratch);
  s.mask = entries - 1;
  s.list_cap = (unsigned)list_cap;
  unsigned counters[kPdCounters] = {0, 0, 0, 0};
  hipError_t e = hipMemcpyAsync(d_off, pose_offset, p_off.bytes(), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && n_poses > 0) e = hipMemcpyAsync(d_xy, pose_xy, (size_t)2 * n_poses * sizeof(double), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_cls, cls.data(), p_cls.bytes(), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_classes, classes.data(), p_classes.bytes(), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(s.keys, 0xFF, p_keys.bytes(), c->stream);  // pv::kEmptyKey
  if (e == hipSuccess) e = hipMemsetAsync(s.counters, 0, p_cnt.bytes(), c->stream);
  if (e == hipSuccess) e = ensure_mask(c);
  const size_t per = (size_t)g.rows * g.cols;
  if (e == hipSuccess)
    e = launch_path_discs(g, s, d_classes, c->L.trav + per * map, c->L.untrav + per * map, c->params.fp_default,
                          c->check_inclination ? c->lmem.robot_slope.as<float>() + per * map : nullptr, n_paths, d_off, d_xy, d_cls, d_safe, d_trav, d_st,
                          c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(is_safe, d_safe, p_safe.bytes(), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(traversability, d_trav, p_trav.bytes(), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(status, d_st, p_st.bytes(), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(counters, s.counters, p_cnt.bytes(), hipMemcpyDeviceToHost, c->stream);
  const hipError_t e_sync = hipStreamSynchronize(c->stream);  // (also before the tables of this call alone are freed)
  if (e == hipSuccess) e = e_sync;
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(TE_ERR_HIP, "te_check_footprint_paths_radius: %s", hipGetErrorString(e));
  }
  // (internal errors -- no HIP call failed: the plan of te_path_visit.h and the kernels' walk disagree; the outputs are not valid)
  if (counters[kPdOverflow])
    return fail(TE_ERR_UNSUPPORTED, "te_check_footprint_paths_radius: internal error: the memo of %llu entries (work list %zu) overflowed", (unsigned long long)entries, list_cap);
  if (counters[kPdVisits] != n_visits)
    return fail(TE_ERR_UNSUPPORTED, "te_check_footprint_paths_radius: internal error: the kernels visited %u centres, the plan counted %llu", counters[kPdVisits], n_visits);
  if (stats) {
    stats->n_visits = (int)counters[kPdVisits];
    stats->n_discs = (int)counters[kPdDiscs];
    stats->n_radius_classes = (int)uniq.size();
  }
  return TE_OK;
}

int te_check_footprint_paths(te_ctx* c, int map, int n_paths, const int* pose_offset, const double* pose_xy,
                             unsigned char* is_safe, double* traversability, int* status) {
  if (!c || n_paths < 0 || (n_paths > 0 && (!pose_offset || !pose_xy || !is_safe || !traversability || !status)))
    return fail(TE_ERR_INVALID_ARG, "te_check_footprint_paths: NULL argument");
  CtxLock lk(c);
  if (!c->have_geo || !c->st.footprint_done())
    return fail(TE_ERR_NOT_READY, "te_check_footprint_paths: run the chain with the footprint pass first");
  if (map < 0 || map >= c->geo.batch) return fail(TE_ERR_INVALID_ARG, "te_check_footprint_paths: map %d of %d", map, c->geo.batch);
  if (c->check_inclination && !c->st.have_robot_slope())
    return fail(TE_ERR_NOT_READY, "te_check_footprint_paths: check_robot_inclination is set but the layer robot_slope was never uploaded");
  if (n_paths == 0) return TE_OK;
  const int n_poses = pose_offset[n_paths];
  if (pose_offset[0] != 0 || n_poses < 0) return fail(TE_ERR_INVALID_ARG, "te_check_footprint_paths: bad pose offsets");
  for (int k = 0; k < n_paths; ++k)
    if (pose_offset[k + 1] < pose_offset[k]) return fail(TE_ERR_INVALID_ARG, "te_check_footprint_paths: bad pose offsets");
  HIP_TRY(hipSetDevice(c->device));
  // staging buffers for this call (paths are small: a few KB .. MB)
  Carve cv;
  const auto p_off = cv.add<int>((size_t)n_paths + 1);
  const auto p_xy = cv.add<double>((size_t)2 * (n_poses > 0 ? n_poses : 1));
  const auto p_trav = cv.add<double>(n_paths);
  const auto p_st = cv.add<int>(n_paths);
  const auto p_safe = cv.add<unsigned char>(n_paths);
  DevBuf tmp;
  HIP_TRY(tmp.once(cv.total));
  int* d_off = p_off.in(tmp);
  double* d_xy = p_xy.in(tmp);
  double* d_trav = p_trav.in(tmp);
  int* d_st = p_st.in(tmp);
  unsigned char* d_safe = p_safe.in(tmp);
  hipError_t e = hipMemcpyAsync(d_off, pose_offset, p_off.bytes(), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && n_poses > 0) e = hipMemcpyAsync(d_xy, pose_xy, (size_t)2 * n_poses * sizeof(double), hipMemcpyHostToDevice, c->stream);
  const size_t per = (size_t)c->geo.rows * c->geo.cols;
  if (e == hipSuccess)
    e = launch_check_circular_paths(c->geo, c->L.footprint + per * map, c->params.fp_default,
                                    c->check_inclination ? c->lmem.robot_slope.as<float>() + per * map : nullptr, n_paths, d_off, d_xy, d_safe,
                                    d_trav, d_st, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(is_safe, d_safe, p_safe.bytes(), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(traversability, d_trav, p_trav.bytes(), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(status, d_st, p_st.bytes(), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(TE_ERR_HIP, "te_check_footprint_paths: %s", hipGetErrorString(e));
  return TE_OK;
}

int te_set_check_robot_inclination(te_ctx* c, int enabled) {
  if (!c) return fail(TE_ERR_INVALID_ARG, "te_set_check_robot_inclination: NULL");
  CtxLock lk(c);
  c->check_inclination = enabled != 0;
  return TE_OK;
}

namespace {
// batched checkInclination on the resident robot_slope layer of map `map`; c->mu held
int check_inclination_locked(te_ctx* c, int map, int n, const double* start_end_xy, unsigned char* ok, int* status,
                             const char* who) {
  if (!c->have_geo || !c->st.have_robot_slope()) return fail(TE_ERR_NOT_READY, "%s: upload the layer robot_slope first", who);
  if (map < 0 || map >= c->geo.batch) return fail(TE_ERR_INVALID_ARG, "%s: map %d of %d", who, map, c->geo.batch);
  if (n == 0) return TE_OK;
  HIP_TRY(hipSetDevice(c->device));
  Carve cv;
  const auto p_seg = cv.add<double>((size_t)4 * n);
  const auto p_st = cv.add<int>(n);
  const auto p_ok = cv.add<unsigned char>(n);
  DevBuf tmp;
  HIP_TRY(tmp.once(cv.total));
  const size_t per = (size_t)c->geo.rows * c->geo.cols;
  hipError_t e = hipMemcpyAsync(p_seg.in(tmp), start_end_xy, p_seg.bytes(), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess)
    e = launch_check_inclination(c->geo, c->lmem.robot_slope.as<float>() + per * map, n, p_seg.in(tmp), p_ok.in(tmp), p_st.in(tmp), c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(ok, p_ok.in(tmp), p_ok.bytes(), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(status, p_st.in(tmp), p_st.bytes(), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(TE_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
  return TE_OK;
}
}  // namespace

int te_check_inclination(te_ctx* c, int map, int n_segments, const double* start_end_xy, unsigned char* ok, int* status) {
  if (!c || n_segments < 0 || (n_segments > 0 && (!start_end_xy || !ok || !status)))
    return fail(TE_ERR_INVALID_ARG, "te_check_inclination: NULL argument");
  CtxLock lk(c);
  return check_inclination_locked(c, map, n_segments, start_end_xy, ok, status, "te_check_inclination");
}

int te_run_polygon_footprint(te_ctx* c, int n_points, const double* points_xy, double yaw) {
  if (!c || !points_xy) return fail(TE_ERR_INVALID_ARG, "te_run_polygon_footprint: NULL");
  if (n_points < 1 || n_points > TE_MAX_POLYGON_VERTICES)
    return fail(TE_ERR_INVALID_ARG, "te_run_polygon_footprint: %d footprint points (1..%d)", n_points, TE_MAX_POLYGON_VERTICES);
  if (!isfinite(yaw)) return fail(TE_ERR_INVALID_ARG, "te_run_polygon_footprint: yaw is not finite");
  for (int k = 0; k < 2 * n_points; ++k)
    if (!isfinite(points_xy[k])) return fail(TE_ERR_INVALID_ARG, "te_run_polygon_footprint: footprint point %d is not finite", k / 2);
  CtxLock lk(c);
  if (!c->have_geo || !c->st.footprint_done())
    return fail(TE_ERR_NOT_READY, "te_run_polygon_footprint: run the chain with the footprint pass first (it marks the untraversable cells)");
  if (c->geo.cols > 65535) return fail(TE_ERR_UNSUPPORTED, "te_run_polygon_footprint: more than 65535 columns");
  HIP_TRY(hipSetDevice(c->device));
  Carve poly;
  poly.add<float>(c->layer_elems);
  const auto p_rot = poly.add<float>(c->layer_elems);
  if (const hipError_t e = c->lmem.poly.once(poly.total))
    return fail(TE_ERR_HIP, "te_run_polygon_footprint: hipMalloc(%zu bytes): %s", poly.total, hipGetErrorString(e));
  float* const poly_x = c->lmem.poly.as<float>();
  c->poly_rot = p_rot.in(c->lmem.poly);
  PolygonArgs a;
  memset(&a, 0, sizeof(a));
  a.n = n_points;
  a.def = c->params.fp_default;
  rotate_footprint(n_points, points_xy, 0.0, a.off[0]);
  rotate_footprint(n_points, points_xy, yaw, a.off[1]);
  // offset tables (te_polygon.hip); polygons that do not fit the table format, or te_set_option(TE_OPT_POLYGON_PER_CELL) (a debugging
  // aid: both kernels give identical layers), take the kernel that evaluates every cell of every bounding box
  PolygonTables tabs;
  HIP_TRY(ensure_mask(c));  // (a score layer written since the footprint pass: the mask is rebuilt from the scores now resident)
  HIP_TRY(hipStreamSynchronize(c->stream));  // the previous call's table upload has been consumed
  c->poly_stream_host.clear();
  bool table = !c->opt_polygon_per_cell;
  for (int w = 0; w < 2 && table; ++w) table = build_polygon_table(c->geo, n_points, a.off[w], c->poly_stream_host, tabs.t[w]);
  if (!table) {
    HIP_TRY(launch_polygon_footprint(c->geo, a, c->L.trav, c->L.untrav, poly_x, c->poly_rot, c->stream));
    return TE_OK;
  }
  if (c->poly_stream_host.empty()) c->poly_stream_host.push_back(0);
  DevBuf& stream_tab = c->lmem.poly_stream;  // (grown with room to spare: the tables' size moves with the yaw)
  const size_t words = c->poly_stream_host.size();
  if (stream_tab.bytes < words * sizeof(unsigned))
    if (const hipError_t e = stream_tab.reserve((words + 1024) * sizeof(unsigned), c->stream))
      return fail(TE_ERR_HIP, "te_run_polygon_footprint: hipMalloc: %s", hipGetErrorString(e));
  HIP_TRY(hipMemcpyAsync(stream_tab.p, c->poly_stream_host.data(), words * sizeof(unsigned), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(launch_polygon_footprint_table(c->geo, a, tabs, stream_tab.as<unsigned>(), c->L.trav, c->L.untrav, poly_x, c->poly_rot,
                                         c->stream));
  return TE_OK;
}

namespace {
// isTraversable(polygon) for a batch of validated polygons; context locked, footprint pass done (the mask is rebuilt here
// when a score layer was written since: ensure_mask)
int polygons_traversable_locked(te_ctx* c, int map, int n_polygons, const int* vertex_offset, const double* vertex_xy,
                                unsigned char* is_traversable, double* traversability, const char* who) {
  if (n_polygons == 0) return TE_OK;
  const int n_vert = vertex_offset[n_polygons];
  HIP_TRY(hipSetDevice(c->device));
  Carve cv;
  const auto p_off = cv.add<int>((size_t)n_polygons + 1);
  const auto p_xy = cv.add<double>((size_t)2 * n_vert);
  const auto p_trav = cv.add<double>(n_polygons);
  const auto p_ok = cv.add<unsigned char>(n_polygons);
  DevBuf tmp;
  HIP_TRY(tmp.once(cv.total));
  int* d_off = p_off.in(tmp);
  double* d_xy = p_xy.in(tmp);
  double* d_trav = p_trav.in(tmp);
  unsigned char* d_ok = p_ok.in(tmp);
  const size_t per = (size_t)c->geo.rows * c->geo.cols;
  hipError_t e = ensure_mask(c);
  if (e == hipSuccess) e = hipMemcpyAsync(d_off, vertex_offset, p_off.bytes(), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_xy, vertex_xy, p_xy.bytes(), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess)
    e = launch_polygons_traversable(c->geo, c->params.fp_default, n_polygons, d_off, d_xy, c->L.trav + per * map,
                                    c->L.untrav + per * map, d_ok, d_trav, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(is_traversable, d_ok, p_ok.bytes(), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(traversability, d_trav, p_trav.bytes(), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(TE_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
  return TE_OK;
}
}  // namespace

int te_polygons_traversable(te_ctx* c, int map, int n_polygons, const int* vertex_offset, const double* vertex_xy,
                            unsigned char* is_traversable, double* traversability) {
  if (!c || n_polygons < 0 || (n_polygons > 0 && (!vertex_offset || !vertex_xy || !is_traversable || !traversability)))
    return fail(TE_ERR_INVALID_ARG, "te_polygons_traversable: NULL argument");
  CtxLock lk(c);
  if (!c->have_geo || !c->st.footprint_done())
    return fail(TE_ERR_NOT_READY, "te_polygons_traversable: run the chain with the footprint pass first (it marks the untraversable cells)");
  if (map < 0 || map >= c->geo.batch) return fail(TE_ERR_INVALID_ARG, "te_polygons_traversable: map %d of %d", map, c->geo.batch);
  if (n_polygons == 0) return TE_OK;
  if (vertex_offset[0] != 0) return fail(TE_ERR_INVALID_ARG, "te_polygons_traversable: bad vertex offsets");
  for (int k = 0; k < n_polygons; ++k)
    if (vertex_offset[k + 1] <= vertex_offset[k])
      return fail(TE_ERR_INVALID_ARG, "te_polygons_traversable: polygon %d has no vertices (or the offsets decrease)", k);
  const int n_vert = vertex_offset[n_polygons];
  for (long k = 0; k < 2L * n_vert; ++k)
    if (!isfinite(vertex_xy[k])) return fail(TE_ERR_INVALID_ARG, "te_polygons_traversable: vertex %ld is not finite", k / 2);
  return polygons_traversable_locked(c, map, n_polygons, vertex_offset, vertex_xy, is_traversable, traversability,
                                     "te_polygons_traversable");
}

int te_polygon_untraversable_hull(te_ctx* c, int map, int n_vertices, const double* vertex_xy, unsigned char* is_traversable,
                                  double* traversability, int cap_vertices, int* n_hull, double* hull_xy) {
  if (!c || !vertex_xy || !is_traversable || !traversability || !n_hull || cap_vertices < 0 || (cap_vertices > 0 && !hull_xy))
    return fail(TE_ERR_INVALID_ARG, "te_polygon_untraversable_hull: NULL argument");
  if (n_vertices < 1) return fail(TE_ERR_INVALID_ARG, "te_polygon_untraversable_hull: a polygon needs at least one vertex");
  for (long k = 0; k < 2L * n_vertices; ++k)
    if (!isfinite(vertex_xy[k])) return fail(TE_ERR_INVALID_ARG, "te_polygon_untraversable_hull: vertex %ld is not finite", k / 2);
  CtxLock lk(c);
  if (!c->have_geo || !c->st.footprint_done())
    return fail(TE_ERR_NOT_READY, "te_polygon_untraversable_hull: run the chain with the footprint pass first (it marks the untraversable cells)");
  if (map < 0 || map >= c->geo.batch) return fail(TE_ERR_INVALID_ARG, "te_polygon_untraversable_hull: map %d of %d", map, c->geo.batch);
  *n_hull = 0;
  const int off[2] = {0, n_vertices};
  const int rc = polygons_traversable_locked(c, map, 1, off, vertex_xy, is_traversable, traversability, "te_polygon_untraversable_hull");
  if (rc != TE_OK || *is_traversable) return rc;  // :635-636 traversable: the empty polygon
  // untraversable: the rows of the bounding box that hold untraversable cells, then the hull on the host
  HIP_TRY(hipSetDevice(c->device));
  Carve cv;
  const auto p_xy = cv.add<double>((size_t)2 * n_vertices);
  const auto p_rows = cv.add<double>((size_t)5 * c->geo.rows);
  DevBuf tmp;
  HIP_TRY(tmp.once(cv.total));
  std::vector<double> rows5((size_t)5 * c->geo.rows);
  const size_t per = (size_t)c->geo.rows * c->geo.cols;
  hipError_t e = ensure_mask(c);  // (built by polygons_traversable_locked above: nothing to do)
  if (e == hipSuccess) e = hipMemcpyAsync(p_xy.in(tmp), vertex_xy, p_xy.bytes(), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = launch_polygon_untraversable_rows(c->geo, n_vertices, p_xy.in(tmp), c->L.untrav + per * map, p_rows.in(tmp), c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(rows5.data(), p_rows.in(tmp), p_rows.bytes(), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(TE_ERR_HIP, "te_polygon_untraversable_hull: %s", hipGetErrorString(e));
  std::vector<double> hull;
  untraversable_hull_from_rows(c->geo.rows, rows5.data(), hull);
  *n_hull = (int)(hull.size() / 2);
  if (*n_hull > cap_vertices)
    return fail(TE_ERR_INVALID_ARG, "te_polygon_untraversable_hull: the hull has %d vertices, room for %d", *n_hull, cap_vertices);
  if (!hull.empty()) memcpy(hull_xy, hull.data(), hull.size() * sizeof(double));
  return TE_OK;
}

int te_check_polygon_footprint_paths(te_ctx* c, int map, int n_paths, const int* pose_offset, const double* poses, int n_points,
                                     const double* points_xyz, const unsigned char* conservative, unsigned char* is_safe,
                                     double* traversability, double* area, int* status) {
  if (!c || n_paths < 0 || !points_xyz ||
      (n_paths > 0 && (!pose_offset || !poses || !is_safe || !traversability || !area || !status)))
    return fail(TE_ERR_INVALID_ARG, "te_check_polygon_footprint_paths: NULL argument");
  if (n_points < 1 || n_points > TE_MAX_POLYGON_VERTICES)
    return fail(TE_ERR_INVALID_ARG, "te_check_polygon_footprint_paths: %d footprint points (1..%d)", n_points, TE_MAX_POLYGON_VERTICES);
  for (int k = 0; k < 3 * n_points; ++k)
    if (!isfinite(points_xyz[k])) return fail(TE_ERR_INVALID_ARG, "te_check_polygon_footprint_paths: footprint point %d is not finite", k / 3);
  CtxLock lk(c);
  if (!c->have_geo || !c->st.footprint_done())
    return fail(TE_ERR_NOT_READY, "te_check_polygon_footprint_paths: run the chain with the footprint pass first (it marks the untraversable cells)");
  if (map < 0 || map >= c->geo.batch) return fail(TE_ERR_INVALID_ARG, "te_check_polygon_footprint_paths: map %d of %d", map, c->geo.batch);
  if (c->check_inclination && !c->st.have_robot_slope())
    return fail(TE_ERR_NOT_READY, "te_check_polygon_footprint_paths: check_robot_inclination is set but the layer robot_slope was never uploaded");
  if (n_paths == 0) return TE_OK;
  if (pose_offset[0] != 0) return fail(TE_ERR_INVALID_ARG, "te_check_polygon_footprint_paths: bad pose offsets");
  for (int k = 0; k < n_paths; ++k)
    if (pose_offset[k + 1] < pose_offset[k]) return fail(TE_ERR_INVALID_ARG, "te_check_polygon_footprint_paths: bad pose offsets");
  for (long k = 0; k < 7L * pose_offset[n_paths]; ++k)
    if (!isfinite(poses[k])) return fail(TE_ERR_INVALID_ARG, "te_check_polygon_footprint_paths: pose %ld is not finite", k / 7);
  // the polygons of all paths: built on the host (hulls, areas), in chunks on a few threads for large requests
  const int n_chunks = n_paths >= 4096 ? std::min<int>(16, std::max(1u, std::thread::hardware_concurrency())) : 1;
  std::vector<PathPolygons> chunk(n_chunks);
  auto first_of = [&](int q) { return (int)((long)n_paths * q / n_chunks); };
  {
    std::vector<std::thread> workers;
    for (int q = 1; q < n_chunks; ++q)
      workers.emplace_back([&, q]() {
        const int k0 = first_of(q);
        build_path_polygons(first_of(q + 1) - k0, pose_offset + k0, poses, n_points, points_xyz,
                            conservative ? conservative + k0 : nullptr, chunk[q]);
      });
    build_path_polygons(first_of(1), pose_offset, poses, n_points, points_xyz, conservative, chunk[0]);
    for (std::thread& w : workers) w.join();
  }
  // checkRobotInclination_ (:526-528, :553-557): one checkInclination per pose of a one-pose path / per segment
  // otherwise, all of them in one launch; incl_first[k] = index of path k's first test
  std::vector<unsigned char> incl_ok;
  std::vector<int> incl_st, incl_first;
  if (c->check_inclination) {
    incl_first.assign((size_t)n_paths + 1, 0);
    std::vector<double> seg;
    for (int k = 0; k < n_paths; ++k) {
      const int n = pose_offset[k + 1] - pose_offset[k];
      const double* q = poses + 7 * (size_t)pose_offset[k];
      if (n == 1) {
        seg.insert(seg.end(), {q[0], q[1], q[0], q[1]});
      } else {
        for (int i = 1; i < n; ++i) seg.insert(seg.end(), {q[7 * (i - 1)], q[7 * (i - 1) + 1], q[7 * i], q[7 * i + 1]});
      }
      incl_first[k + 1] = (int)(seg.size() / 4);
    }
    const int n_seg = incl_first[n_paths];
    incl_ok.assign(n_seg > 0 ? n_seg : 1, 0);
    incl_st.assign(n_seg > 0 ? n_seg : 1, 0);
    const int rc = check_inclination_locked(c, map, n_seg, seg.data(), incl_ok.data(), incl_st.data(),
                                            "te_check_polygon_footprint_paths");
    if (rc != TE_OK) return rc;
  }
  std::vector<unsigned char> ok;
  std::vector<double> val;
  for (int q = 0; q < n_chunks; ++q) {
    const PathPolygons& pp = chunk[q];
    const int k0 = first_of(q), nk = first_of(q + 1) - k0;
    const int n_poly = (int)pp.area.size();
    ok.assign(n_poly > 0 ? n_poly : 1, 0);
    val.assign(n_poly > 0 ? n_poly : 1, 0.0);
    const int rc = polygons_traversable_locked(c, map, n_poly, pp.vertex_offset.data(), pp.vertex_xy.data(), ok.data(),
                                               val.data(), "te_check_polygon_footprint_paths");
    if (rc != TE_OK) return rc;
    // the loop of :480-580 over the precomputed polygons; a path stops at its first untraversable polygon and keeps
    // the partial traversability / area, like `result` in the reference
    for (int kk = 0; kk < nk; ++kk) {
      const int k = k0 + kk;
      is_safe[k] = 0;
      traversability[k] = 0.0;
      area[k] = 0.0;
      status[k] = pp.status[kk];
      if (pp.status[kk] == 2) continue;
      const int n = pose_offset[k + 1] - pose_offset[k];
      bool good = true;
      for (int s = 0; s < pp.count[kk] && good; ++s) {
        const int g = pp.first[kk] + s;
        if (c->check_inclination && !incl_ok[incl_first[k] + s]) {  // before isTraversable (:553-557); the partial result stays
          status[k] = incl_st[incl_first[k] + s];
          good = false;
          break;
        }
        if (!ok[g]) {
          good = false;
          break;
        }
        if (n == 1 || s == 0) {  // :543-544, :576-577
          area[k] = pp.area[g];
          traversability[k] = val[g];
        } else {  // :570-575
          const double area_previous = area[k];
          const double area_polygon = pp.area[g] - pp.area_previous[g];
          area[k] += area_polygon;
          traversability[k] = (area_polygon * val[g] + area_previous * traversability[k]) / area[k];
        }
      }
      if (good && pp.status[kk] == 0) is_safe[k] = 1;
    }
  }
  return TE_OK;
}

int te_path_polygons(int n_paths, const int* pose_offset, const double* poses, int n_points, const double* points_xyz,
                     const unsigned char* conservative, int cap_polygons, int cap_vertices, int* n_polygons, int* n_vertices,
                     int* polygon_first, int* vertex_offset, double* vertex_xy, double* area) {
  if (n_paths < 0 || !n_polygons || !n_vertices || !points_xyz || (n_paths > 0 && (!pose_offset || !poses)))
    return fail(TE_ERR_INVALID_ARG, "te_path_polygons: NULL argument");
  if (n_points < 1 || n_points > TE_MAX_POLYGON_VERTICES)
    return fail(TE_ERR_INVALID_ARG, "te_path_polygons: %d footprint points (1..%d)", n_points, TE_MAX_POLYGON_VERTICES);
  for (int k = 0; k < n_paths; ++k)
    if (pose_offset[0] != 0 || pose_offset[k + 1] < pose_offset[k]) return fail(TE_ERR_INVALID_ARG, "te_path_polygons: bad pose offsets");
  // the same input checks as te_check_polygon_footprint_paths: a NaN pose would otherwise come back as a degenerate hull
  for (int k = 0; k < 3 * n_points; ++k)
    if (!isfinite(points_xyz[k])) return fail(TE_ERR_INVALID_ARG, "te_path_polygons: footprint point %d is not finite", k / 3);
  for (long k = 0; n_paths > 0 && k < 7L * pose_offset[n_paths]; ++k)
    if (!isfinite(poses[k])) return fail(TE_ERR_INVALID_ARG, "te_path_polygons: pose %ld is not finite", k / 7);
  PathPolygons pp;
  build_path_polygons(n_paths, pose_offset, poses, n_points, points_xyz, conservative, pp);
  *n_polygons = (int)pp.area.size();
  *n_vertices = pp.vertex_offset.back();
  if (*n_polygons > cap_polygons || *n_vertices > cap_vertices)
    return fail(TE_ERR_INVALID_ARG, "te_path_polygons: %d polygons / %d vertices do not fit the buffers (%d / %d)", *n_polygons,
                *n_vertices, cap_polygons, cap_vertices);
  // (nothing to write: a sizing call, or paths without poses -- the buffers may be NULL then)
  if (!polygon_first || !vertex_offset || (*n_vertices && !vertex_xy) || (*n_polygons && !area))
    return fail(TE_ERR_INVALID_ARG, "te_path_polygons: NULL output");
  for (int k = 0; k < n_paths; ++k) polygon_first[k] = pp.first[k];
  polygon_first[n_paths] = *n_polygons;
  memcpy(vertex_offset, pp.vertex_offset.data(), pp.vertex_offset.size() * sizeof(int));
  if (*n_vertices) memcpy(vertex_xy, pp.vertex_xy.data(), pp.vertex_xy.size() * sizeof(double));
  if (*n_polygons) memcpy(area, pp.area.data(), pp.area.size() * sizeof(double));
  return TE_OK;
}

}  // extern "C"
