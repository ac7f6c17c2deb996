// te_ctx.h -- the context behind the C-ABI (struct te_ctx) and what the translation units of the shim share:
//   te_shim.hip      context, parameters, geometry, tables, the launch entry points (te_run_*), te_sync, timing
//   te_transfer.hip  uploads / downloads: whole layers, tiles, circular-buffer order, GridMap messages, prefetch, pinning
//   te_paths_api.hip path checks, inclination, polygon footprint layers (N2, N3)
//   te_multi.hip     the batch axis over several contexts / devices (te_shard_range, te_bcast_params over RCCL, *_multi)
// The tables the shim uploads are built by plain C++ headers the CPU checks compile too: te_disc.h (discs, tie circle, clip
// table), te_disc_table.h (discs of any radius), te_fp_table.h (footprint spiral and inner rings).
// No CPU fallback of any kind: without a gfx950 device te_create() fails with TE_ERR_NO_DEVICE.
//
// Device memory: every allocation the context keeps is a DevBuf (te_devbuf.h) declared in one of two groups, and the group
// says when it is freed -- te_ctx::LayerMem with the layers (free_layers: te_set_geometry to another shape, te_destroy),
// te_ctx::CtxMem with the context (te_destroy).  Each group is released in one statement, so a buffer declared there
// cannot be forgotten.  What must stay next to a release are the pointers DERIVED from a buffer: they are cleared or
// re-derived wherever their buffer is released or regrown (c->fp.any_*, Disc::tab, Layers::tie_scratch / hole_queue,
// c->poly_rot, c->face_flags and the slab's layer pointers in c->L).  A call's own temporaries are local DevBufs.
#pragma once
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <condition_variable>
#include <dlfcn.h>
#include <functional>
#include <chrono>
#include <mutex>
#include <new>
#include <optional>
#include <thread>
#include <vector>

#include <cstdlib>
#include "te_ctx_state.h"
#include "te_devbuf.h"
#include "te_disc_table.h"
#include "te_internal.h"
#include "te_layer_call.h"
#include "te_msg.h"
#include "te_user_layers.h"

struct te_ctx;

namespace te {
namespace shim {
// records the message te_last_error() returns (thread-local) and hands `code` back
int fail(int code, const char* fmt, ...);
}  // namespace shim
}  // namespace te

#define HIP_TRY(expr)                                                                            \
  do {                                                                                           \
    hipError_t e__ = (expr);                                                                     \
    if (e__ != hipSuccess) {                                                                     \
      (void)hipGetLastError(); /* the runtime's last-error slot is sticky: later launches check it */ \
      return ::te::shim::fail(TE_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e__));                          \
    }                                                                                            \
  } while (0)

struct te_ctx {
  std::mutex mu;
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipStream_t aux_stream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  te_params params;
  bool have_params = false, have_geo = false;
  // which cached results still describe the resident layers: every fact and every transition in te_ctx_state.h
  te::CtxState st;
  // te_check_footprint_paths_radius (te_path_discs.hip): the spiral table of one radius class on the device, by (radius,
  // offset, resolution, map size)
  struct PdTable {
    double radius = 0.0, offset = 0.0, res = 0.0;
    int rows = 0, cols = 0;  // (the clip)
    te::DevBuf dev;          // FpEntry [n_spiral]
    int n_spiral = 0;
    unsigned long long used = 0;  // pd_clock at its last use
  };
  static constexpr int kPdTables = 16;
  // Device memory freed with the layers (free_layers).  The "grown" ones hold the largest request so far.
  struct LayerMem {
    te::DevBuf slab;         // te_slab.h: the layers of c->L, the mask, the lists and flag grids of the footprint pass, c->face_flags
    te::DevBuf poly;         // traversability_x, and behind it traversability_rot (c->poly_rot); made by the first te_run_polygon_footprint
    te::DevBuf poly_stream;  // offset tables of the two footprint polygons (device copy of poly_stream_host); grown
    te::DevBuf robot_slope;  // layer robot_slope (checkInclination); allocated by its first upload, NaN until written
    te::DevBuf tie_scratch;  // one float per cell: the step filter at a tie radius (allocated when a launch first needs it)
    te::DevBuf img_stage;    // te_upload_image: the raw image bytes (te_image.hip converts and transposes them into a layer); grown
    // te_download_occupancy (te_occupancy.hip) / te_download_cloud (te_cloud.hip): the converted cells / the block counts,
    // block offsets and compacted records; grown
    te::DevBuf occ_out, cloud_counts, cloud_out;
    // te_run_expression (te_expr.hip): the per-block partials of its reductions and, behind them, the folded results per
    // (map, reduction); grown
    te::DevBuf expr_scratch;
    // te_run_median_fill (te_median.hip), each allocated when a call first needs it: the shouldFill mask of the last call,
    // one byte per cell of the batch (te_download_fill_mask; which maps hold one: fill_mask_valid); the two scratch masks of
    // its mask passes, behind each other; the copy of the input layer a call with in_layer == out_layer reads; the general
    // route's counts and list
    te::DevBuf median_mask, median_tmp, median_copy, median_any;
    // te_run_radius_filter (te_radius.hip): the copy of the input layer a call with in_layer == out_layer reads
    te::DevBuf radius_copy;
    // te_run_window_expression (te_window_expr.hip): the copy of the input layer a call with in_layer == out_layer reads
    te::DevBuf window_copy;
    // te_run_distance (te_distance.hip): the column distances of pass 1, 16 bits per cell of the rectangle pass 2 reads; grown
    te::DevBuf distance_g;
    // te_run_components / te_run_reachable (te_components.hip): a label and a count of 32 bits each per cell of the call; grown
    te::DevBuf components_scratch;
    // te_move_map (te_move.hip): one float layer of one map, the out-of-place target of a shift (te_slab.h: move_scratch_bytes);
    // allocated by the first move that needs it
    te::DevBuf move_scratch;
    // the user layers (te_add_layer; te_user_layers.h holds their names, which outlive this memory): one float layer each,
    // allocated and filled with NaN by the first write (ensure_input_layer), released one by one by te_remove_layer
    te::DevBuf user[TE_MAX_USER_LAYERS];
    // the circular footprint at any reach (te_footprint_any.hip): its tables and its prefix-sum scratch ([batch][cols][rows + 1]
    // doubles, then as many unsigned), allocated when the footprint tables are rebuilt for that route; c->fp.any_* point into them
    struct FpAny {
      te::DevBuf tab, prefix;
    } fpa;
    // te_check_footprint_paths_radius: at most kPdTables spiral tables, the least recently used one replaced (they are
    // clipped to the map); pd_scratch: the call's staging buffers and memo, grown
    PdTable pd_tables[kPdTables];
    te::DevBuf pd_scratch;
  } lmem;
  // Device memory freed with the context (te_destroy)
  struct CtxMem {
    te::DevBuf spiral;         // uint32_t [kMaxSpiral]: the footprint spiral of reach <= 20, packed (fp_pack)
    te::DevBuf count;          // two counters of k_count_invalid
    te::DevBuf hole_queue;     // scratch of k_normals3's sparse-hole march (allocated when a launch first picks it)
    te::DevBuf clip_table, fp_clip_table;
    te::DevBuf fa_tab;         // the tables of the filter discs of any radius (Disc::tab points into it); grown
    te::DevBuf tile_in[2], tile_out[2];  // the device staging of in_slot / out_slot; grown
    // te_run_radius_filter: the window table of the last call (device copy of radius_tab_host; grown) and its two block counts
    te::DevBuf radius_tab, radius_counts;
    te::DevBuf window_counts;  // te_run_window_expression: its two block counts
    te::DevBuf components_counts;  // te_run_components / te_run_reachable: the four totals of te_components_stats
  } cmem;
  float* poly_rot = nullptr;  // (derived: lmem.poly)
  bool check_inclination = false;  // footprint/check_robot_inclination (:114)
  std::vector<unsigned> poly_stream_host;  // stays alive until the asynchronous upload has been consumed
  te::user::Table user;  // names of the user layers (their memory: lmem.user)
  te::Geo geo;
  te::ChainParams cp;
  te::FootprintParams fp;
  te::Layers L;
  size_t layer_elems = 0;
  unsigned long long pd_clock = 0;  // (lmem.pd_tables)
  // te_set_option: choices between kernels that give identical results (tests reach both; never read from the environment)
  int opt_fb_walk = 0, opt_fb_blocks_per_cu = 0, opt_polygon_per_cell = 0, opt_graph = 0, opt_bcast_rccl = 0, opt_rank_rule = 0,
      opt_fp_any = 0;
  int opt_normals_raster = 0;  // TE_OPT_NORMALS_ALGORITHM: 1 the raster method (changes the layers: te_ctx_state.h, normals_algorithm_set)
  // TE_OPT_FILTER_ANY_RADIUS (0: discs above 32 cells refused, 1: those take te_filter_any.hip, 2: every disc does), the host
  // tables of the filter discs that route takes (normals, roughness, step windows 1 and 2) and their device copy (cmem.fa_tab),
  // uploaded by rebuild_tables (never inside a launch: whole-map launches are captured)
  int opt_filter_any = 0;
  te::DiscTable fa_host[4];
  // TE_OPT_MEDIAN_ROUTE (te_median_plan.h), and per map of the batch whether lmem.median_mask holds the mask of a
  // te_run_median_fill (empty: of none; cleared by every te_set_geometry)
  int opt_median_route = 0;
  std::vector<uint8_t> fill_mask_valid;
  // TE_OPT_RADIUS_ROUTE (te_radius_plan.h); the host copy of the last call's window table (alive until its asynchronous
  // upload has been consumed) with the (radius, resolution) it was built for; whether a call has left block counts
  int opt_radius_route = 0;
  std::vector<int32_t> radius_tab_host;
  double radius_tab_radius = -1.0, radius_tab_res = 0.0;
  te::DiscTable radius_disc;
  bool radius_counts_valid = false;
  // TE_OPT_WINDOW_EXPR_ROUTE (te_window_plan.h); whether a te_run_window_expression has left block counts
  int opt_window_expr_route = 0;
  bool window_counts_valid = false;
  // TE_OPT_DISTANCE_ROUTE (te_distance_plan.h); the workgroups of pass 2 the last te_run_distance launched on either route
  int opt_distance_route = 0;
  unsigned long long distance_counts[2] = {0, 0};
  bool distance_counts_valid = false;
  // whether a te_run_components or te_run_reachable has left its totals in cmem.components_counts
  bool components_counts_valid = false;
  // face flags (te_face_flags.h): the bytes live in the slab; what they describe: te::CtxState::face_crit
  uint8_t* face_flags = nullptr;
  int opt_face_flags = 1;  // TE_OPT_FACE_FLAGS
  bool tables_ready = false;
  // the circular-footprint tables are built separately: a footprint whose tables do not fit in device memory must not
  // stop the filter chain or the per-plugin entry points, which never use them (the reference has no such coupling)
  bool fp_tables_ready = false;
  int fp_tables_rc = TE_OK;
  char fp_tables_err[256] = "";
  // the launch sequence of a whole-map run, captured once per (flags, parameters, geometry) and replayed
  static constexpr int kGraphs = 4;  // one per flag combination in use
  hipGraphExec_t graph_exec[kGraphs] = {nullptr, nullptr, nullptr, nullptr};
  unsigned graph_flags[kGraphs] = {0, 0, 0, 0};
  int graph_next = 0;
  bool graph_ok = true;  // cleared after a failed capture: direct launches from then on
  // streaming tiles (te_upload_tile_async / te_download_tile_async): copy streams, two device staging slots each way
  struct TileSlot {  // (its device buffer: cmem.tile_in / tile_out)
    hipEvent_t ready = nullptr, freed = nullptr;  // filled / consumed
    bool used = false;
  };
  hipStream_t in_stream = nullptr, out_stream = nullptr;
  TileSlot in_slot[2], out_slot[2];
  int in_next = 0, out_next = 0;
  bool tiles_pending = false;  // te_sync has copy streams to wait for
  te::HostStager stager;           // whole-layer transfers through pageable host buffers (te_stage.hip)
  // te_prefetch_layers: whole-layer uploads on a thread of their own, through a second staging ring and the second copy
  // pool, beside whatever the caller does meanwhile (a filter on other layers, the download of its output)
  te::HostStager prefetcher;
  hipStream_t prefetch_order = nullptr;  // stands in for the compute stream of HostStager::upload
  // (one worker per context, started by the first prefetch and kept: a new thread's first HIP call pays the runtime's
  // per-thread set-up, milliseconds that a 3 ms transfer cannot afford)
  std::thread prefetch_thread;
  std::mutex pf_mu;
  std::condition_variable pf_cv;
  std::function<void()> pf_job;
  bool pf_quit = false;
  bool prefetch_running = false, prefetch_elev = false;  // (prefetch_running: a job is queued or being worked on; under pf_mu)
  // bit TE_LAYER_* of every layer the prefetch in flight is writing (under mu): a call that runs beside a prefetch joins
  // it first if it reads or writes one of them (te_run_filter, te_download_layer*)
  unsigned prefetch_mask = 0;
  std::atomic<int> prefetch_rc{TE_OK};
};

namespace te {
namespace expr {
struct Program;  // te_expr.h
struct Args;     // te_expr_launch.h
}  // namespace expr
namespace shim {
// joins a running prefetch (caller holds c->mu); its result stays in c->prefetch_rc until te_wait_prefetch reports it
void finish_prefetch_locked(te_ctx* c);
// Every entry point takes the context's mutex through this: a prefetch that is still running is finished first -- except
// in the calls that are meant to run beside one (te_run_filter, te_download_layer*, the parameter calls).
struct CtxLock {
  std::lock_guard<std::mutex> lk;
  // beside_prefetch: the call may run while a prefetch is in flight -- unless it touches one of the layers the prefetch is
  // writing (`touches`: bits TE_LAYER_*), in which case it joins it like every other call
  explicit CtxLock(te_ctx* c, bool beside_prefetch = false, unsigned touches = 0) : lk(c->mu) {
    if (!beside_prefetch || (touches & c->prefetch_mask)) finish_prefetch_locked(c);
  }
};
constexpr unsigned bit(int layer) { return layer_bit(layer); }
// counts the invalid cells of the whole elevation layer on the context's stream, builds its face flags, waits for the result
// and records it in c->st (unknown from the start of the call until it has succeeded)
int count_invalid_elevation(te_ctx* c);
// the face flags a mask launch may read now (nullptr: unknown, or switched off)
const uint8_t* usable_face_flags(const te_ctx* c);
float* layer_ptr(te_ctx* c, int layer);
int ensure_input_layer(te_ctx* c, int layer);
// The call contract of the layer filters (te_layer_call.h) on a context: its facts, and a refusal as the entry point's status
// and message -- the one home of each wording.  Caller holds the lock.
te::layer_call::Facts facts_of(const te_ctx* c);
// where a call points, for the messages: maps [map0, map0 + nmaps) (a region form: the map `map0`) and the rectangle
struct CallWhere {
  int map0 = 0, nmaps = 1, max_maps = 0;
  int row0 = 0, col0 = 0, h = 0, w = 0;
};
// TE_OK for an accepted verdict, else fail(v.code, ...)
int refused(const char* who, const te_ctx* c, const te::layer_call::Verdict& v, const CallWhere& at = CallWhere());
// a reference layer, or a user layer that was added: the ids an entry point takes at all
inline bool layer_known(const te_ctx* c, int layer) {
  te::layer_call::Facts f;
  f.user_added = c->user.mask();
  return te::layer_call::known(f, layer);
}
// the layers whose memory comes from their first write (ensure_input_layer): robot_slope and the user layers
inline bool layer_on_demand(const te_ctx* c, int layer) {
  te::layer_call::Facts f;
  f.user_added = c->user.mask();
  return te::layer_call::on_demand(f, layer);
}
// the layer as a download reads it: TE_ERR_INVALID_ARG for an id that is no layer or a reference layer without memory (as ever),
// TE_ERR_NOT_READY for a user layer that is absent
int readable_layer(const char* who, te_ctx* c, int layer, float** out);
// The user names as operands of an expression, copied under the context's mutex (taken and dropped here): an entry point
// compiles its text before it takes its CtxLock.  A layer removed in between is then simply absent.
struct UserNames {
  te::expr::LayerName v[TE_MAX_USER_LAYERS];
  te::user::Table copy;
  int n = 0;
  bool has(int layer) const { return copy.added(layer); }
};
void snapshot_user_names(te_ctx* c, UserNames* out);
// the name of a layer the context knows, for messages
const char* layer_name_of(const te_ctx* c, int layer);
// te_median_api.hip, shared by the device filters: b.reserve with TE_ERR_UNSUPPORTED and a message; the facts of an upload of
// the same values into out_layer
int reserve_scratch(const char* who, te::DevBuf& b, size_t bytes, hipStream_t stream, const char* what);
int note_layer_written(te_ctx* c, int out_layer);
// ... and of the region filters: their checks for one map and one rectangle (the cells of the map behind *in / *out), and the
// facts of te_upload_tile (the elevation) or te_upload_layer (any other layer) afterwards
int region_filter_layers(const char* who, te_ctx* c, int in_layer, int out_layer, int map, int row0, int col0, int h, int w, const float** in, float** out);
void note_region_written(te_ctx* c, int out_layer);
// the rectangle a region call wrote, as its out_rect: row0, col0, height, width
inline void write_rect(const te::region::Rect& r, int out_rect[4]) {
  out_rect[0] = r.i0;
  out_rect[1] = r.j0;
  out_rect[2] = te::region::height(r);
  out_rect[3] = te::region::width(r);
}
// the two block counts a filter left in `counts`, read back (waits for the stream); caller holds the lock
int read_block_counts(te_ctx* c, const te::DevBuf& counts, uint64_t out[2]);
// what te_expr_check and its kin report of a compiled program (te_expr_api.hip)
void fill_expr_info(const te::expr::Program& p, te_expr_info* info);
// te_expr_api.hip, the rectangle form of te_run_expression, shared with te_run_chain_region_expression: compile and refuse
// (a reduction, a text that reads the traversability layer: TE_ERR_UNSUPPORTED) without a context; bind the layers
// (TE_ERR_NOT_READY: one is missing) without a launch; launch on a rectangle of one map and record the facts of
// te_upload_layer_tile(TE_LAYER_TRAVERSABILITY).  The last two under the caller's lock.
// (un: user names that are operands too, or NULL; out_layer: the layer the text writes and therefore must not read)
int region_expression_program(const char* who, const char* text, te::expr::Program* p, const UserNames* un = nullptr, int out_layer = TE_LAYER_TRAVERSABILITY);
int region_expression_args(const char* who, te_ctx* c, const te::expr::Program& p, te::expr::Args* a);
int region_expression_launch(const char* who, te_ctx* c, const te::expr::Program& p, const te::expr::Args& a, int map, int row0, int col0, int h, int w,
                             int out_layer = TE_LAYER_TRAVERSABILITY);
int rebuild_tables(te_ctx* c);
void rebuild_footprint_tables(te_ctx* c);
// destroys the captured whole-map launches: their kernel arguments (tables, grids, the geometry) are baked in
void drop_graph(te_ctx* c);
int sync_tiles(te_ctx* c);  // waits for the copy streams of the streaming-tile calls
int run_whole_locked(te_ctx* c, unsigned flags);

// The event-timed loop of the te_time_*_samples: warmup + iters times `before()` (outside the timed span), ev0, `body()`, ev1,
// and the elapsed time of the last `iters` into ms.  Both return a status; the first that is not TE_OK ends the loop.
// locked: the caller holds the context's lock over the whole loop and has made the device current.  Otherwise `body` is an
// entry point that takes the lock itself, and the loop takes it around its events.
template <class Before, class Body>
int time_samples(te_ctx* c, bool locked, int warmup, int iters, float* ms, Before before, Body body) {
  for (int k = -warmup; k < iters; ++k) {
    {
      std::optional<CtxLock> lk;
      if (!locked) {
        lk.emplace(c);
        HIP_TRY(hipSetDevice(c->device));
      }
      if (const int rc = before()) return rc;
      HIP_TRY(hipEventRecord(c->ev0, c->stream));
    }
    if (const int rc = body()) return rc;
    std::optional<CtxLock> lk;
    if (!locked) lk.emplace(c);
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev1));
    float t = 0.0f;
    HIP_TRY(hipEventElapsedTime(&t, c->ev0, c->ev1));
    if (k >= 0) ms[k] = t;
  }
  return TE_OK;
}
}  // namespace shim
}  // namespace te
