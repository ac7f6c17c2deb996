// te_internal.h -- shared between the C-ABI shim (te_shim.hip) and the gfx950 kernels (te_kernels.hip).
#pragma once
#include <atomic>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include <vector>

#include "te_chain_route.h"
#include "te_disc.h"
#include "te_face_flags.h"
#include "te_fp_route.h"
#include "te_polygon_table.h"
#include "te_slab.h"
#include "travgpu.h"

namespace te {

// Measurement switches: environment variables read once per process, in a LAB build only (-DTE_LAB: build.py --lab ->
// libtravgpu_lab.so, which tools/ load through TRAVGPU_LIB).  In the shipped library they are compile-time constants:
// nothing the product does depends on the environment.  (Choices between kernels with identical results that the tests
// need to reach are part of the C-ABI instead: te_set_option.)
#ifdef TE_LAB
inline int lab_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) : dflt;
}
inline bool lab_flag(const char* name) { return getenv(name) != nullptr; }
#else
constexpr int lab_int(const char*, int dflt) { return dflt; }
constexpr bool lab_flag(const char*) { return false; }
#endif

// A roctx range over the enclosing scope (te_trace.hip): the phases of a launch in `rocprofv3 --marker-trace`.
class TraceRange {
 public:
  explicit TraceRange(const char* name);
  ~TraceRange();
  TraceRange(const TraceRange&) = delete;
  TraceRange& operator=(const TraceRange&) = delete;

 private:
  bool live_;
};
bool trace_available();

// The marching kernels of te_march5.h load the rows above / below a map unconditionally (and stage them as "nothing
// there"): up to the stencil radius above the first row, and the radius plus the prefetch distance below the last.  The
// context's slab therefore starts and ends with this many rows of slack (kSlabGuardRows of te_slab.h, the plan of the slab).
static_assert(kSlabGuardRows == kMaxRadiusCells + 16, "te_slab.h: the guard rows cover the largest radius and the prefetch distance");
constexpr int kMaxSpiral = 4096;     // ordered offsets of the footprint spiral

// (struct Geo, the map geometry as the kernels need it: te_polygon_table.h, plain C++ the CPU checks can include)

struct ChainParams {
  Disc normals, rough, step1, step2;
  int same_rough_disc;  // roughness radius selects the same cells as the normals radius
  int axis;             // normal_vector_positive_axis
  int rank_rule;        // TE_OPT_NORMALS_RANK_RULE: a rank-deficient scatter matrix gives UnitZ (generic normals kernel)
  int raster;           // TE_OPT_NORMALS_ALGORITHM = 1: the raster method (te_normals_raster.hip); the normals disc is not read
  double slope_crit, step_crit, rough_crit;
  int step_ncrit;
  float w_scale, w_slope, w_step, w_rough;
  // what plan_chain_route asks that changes only with the parameters and the geometry (the discs' summaries, the map, the
  // device's CUs, the lab switches): filled by chain_route_template when the tables are rebuilt; a launch adds its own facts
  fast::ChainRouteIn route;
};

// THE CLIP OF A SCORE.  SlopeFilter / RoughnessFilter clip their scores at 0 (SlopeFilter.cpp:77-81, RoughnessFilter.cpp:119-124)
// and the footprint checks treat "score == 0" as a category of its own: checkForSlope / checkForRoughness run -- and
// memoise -- only where the score IS 0 (TraversabilityMap.cpp:869, :897).  A fast tail whose score lands within its own
// error of the clip therefore does not decide the cell: it writes the kExactNaN payload into the slope layer and flags the
// tile, and the fix-up pass settles the cell with the generic arithmetic (gather in the generic order, cyclic Jacobi,
// double acos: bit-identical to the generic kernels and the oracle).  The bands are the fast tails' error bounds in score
// units with a margin of 3, from the parameters (host side):
//   slope:  (float32 acos polynomial + float rounding: 4e-7 rad  +  one float32 ulp of nz: 1.2e-7 / sin(crit) rad) / crit
//   roughness: float32 square root, product and 1/crit: 3 * 2^-23, relative to a score distance of 1 at the clip
constexpr unsigned kExactNaNBits = 0x7fc00001u;  // slope (given normals: roughness) of a cell the fix-up pass must settle exactly
inline float clip_band_slope(double crit) {
  if (!(crit > 0.0)) return 0.0f;
  double s = sin(crit);
  s = s > 1e-3 ? s : 1e-3;
  const double e = 3.0 * (4e-7 + 1.2e-7 / s) / crit;
  return (float)(e < 2e-6 ? 2e-6 : (e > 1e-2 ? 1e-2 : e));
}
inline float clip_band_rough(double crit) { return crit > 0.0 ? 2e-6f : 0.0f; }

constexpr unsigned kDeferCombine = 0x8000u;  // internal launch_chain flag: the footprint mask kernel will write `traversability`

struct Region {  // half-open cell rectangle of one map (or all maps when map < 0)
  int map, i0, j0, i1, j1;
};

struct FootprintParams {
  Disc slope_disc;   // circle(3*res) of checkForSlope / checkForRoughness
  Disc step_disc;    // circle(2.5*res) of checkForStep
  Disc fp_disc;      // circle(radiusMax) of the spiral
  int reach;         // largest |offset| the spiral visits
  int ncrit_slope, ncrit_rough;
  double rmin, rmax, def, max_gap, crit_step;
  int check_rough;
  int n_spiral;      // entries of the ordered spiral table
  // the route of any reach (te_footprint_any.hip): above 20 cells, every reach with TE_OPT_FP_ANY_REACH = 1, or (any == 0,
  // the buffers built all the same) a layer without the bound the double kernels need (te_fp_route.h).  Its
  // tables (te_fp_table.h, clipped to the map) and the prefix-sum scratch are device buffers of the context, allocated
  // when the tables are rebuilt; fp_disc and the shape-specialised tables are not built for a reach above 20 cells.
  int any;              // 1: this route serves the pass
  const int* any_spiral;  // FpEntry [any_n_spiral]: {di, dj, ring, tie}
  const int* any_ints;    // run half-widths [any_R + 1], inner-disc half-widths [any_inner_R + 1], ties [2 any_n_ties]
  double* any_psum;       // [batch][cols][rows + 1]: column prefix sums of T'
  unsigned* any_pcnt;     // [batch][cols][rows + 1]: column prefix counts of untraversable cells
  int any_n_spiral, any_R, any_inner_R, any_n_ties, any_k_inner;
};

struct Layers {
  float* elev;
  float* slope;
  float* step;
  float* rough;
  float* trav;
  float* footprint;
  float* nx;
  float* ny;
  float* nz;
  float* slope_fp;
  float* step_fp;
  float* rough_fp;
  float* step_height;  // temp layer of StepFilter (never leaves the device)
  uint8_t* untrav;     // !isTraversableForFilters per cell
  float* tie_scratch;          // one float per cell: the step filter at a tie radius (te_fast_step.hip); nullptr: not allocated
  unsigned* fp_blocked;        // k_fp_slide4's list of cells whose disc holds an untraversable cell (one entry per cell at most) ...
  unsigned* fp_blocked_count;  // ... [0] entries of the list (some hold kF4NoCell), [1] cells listed, [3] first spiral entry that can be untraversable
                               // in a listed disc, [4] entries of the scratch reserved (k_fp_mask resets [0], [1], [4])
  unsigned* fp_scratch;        // k_fp_slide5 collects a block's cells here (one reservation per block, sized for its whole strip) and copies
                               // them to the list when the strip is done: the list stays dense whatever the reservations
  size_t fp_blocked_cap;       // entries the list holds (cells + fast::fp_list_slack)
  int* block_flags;    // one flag per block of the shape-specialised normals kernel ("needs the fix-up pass")
  uint8_t* untrav_flags;  // one byte per 64 x 4 cells: "holds an untraversable cell" as of the mask kernel's last pass over them (1 until then);
                          // k_fp_slide5 does not fetch the mask bytes of a strip whose flags are all clear
  int* clip_table;     // x/y moments of the normals disc clipped by the map border (build_clip_table)
  // second stream + fork/join events: step filter || normals kernel on whole-map runs (nullptr: sequential)
  hipStream_t aux_stream;
  hipEvent_t ev_fork, ev_join;
  int fb_walk, fb_blocks_per_cu;  // te_set_option: k_fp_blocked's walk (0: by the length of the list, 1: per wavefront, 2: per lane) and grid (0: default)
  int sparse_holes;  // 1: at most a few per mille of the elevation cells are invalid (counted at upload): k_normals3 takes its sparse march
  int no_holes;      // 1: none of them is (counted at upload): the clean march alone, on its slim ring (k_normals3s)
  int skip_clean;    // 1: scattered invalid cells, several per strip on average (sparse march): the clean march is not attempted first
  int short_strips;  // 1: invalid cells counted, too many for the sparse march -- unobserved regions as a rule: k_normals3 cuts the map
                     // into strips of 32 rows, more blocks than resident slots (a strip along the edge of a region takes 2.6x
                     // the time of a clean one and the pass lasted as long as its slowest strip: te_normals3.hip, launch3)
  char* hole_queue;  // its scratch: normals_hole_queue_bytes() (te_normals3.hip), nullptr: the dense march serves
};

// polygon footprints (te_polygon.hip)
struct PolygonArgs {
  int n;
  double def;                                       // traversabilityDefault_
  double off[2][2 * TE_MAX_POLYGON_VERTICES];       // vertex offsets from the centre cell: [0] as given, [1] turned by yaw
};
// (PolygonTable, PolygonTables and build_polygon_table, the offset table of one footprint polygon: te_polygon_table.h)
hipError_t launch_polygon_footprint_table(const Geo& g, const PolygonArgs& a, const PolygonTables& tabs, const unsigned* d_stream,
                                          const float* trav, const uint8_t* untrav, float* out_x, float* out_rot,
                                          hipStream_t stream);
hipError_t launch_polygon_footprint(const Geo& g, const PolygonArgs& a, const float* trav, const uint8_t* untrav, float* out_x,
                                    float* out_rot, hipStream_t stream);
hipError_t launch_polygons_traversable(const Geo& g, double def, int n_polygons, const int* vertex_offset, const double* vertex_xy,
                                       const float* trav, const uint8_t* untrav, unsigned char* is_traversable,
                                       double* traversability, hipStream_t stream);

// isTraversable(polygon, computeUntraversablePolygon = true): per row index of the map (x, y first, y last, y between,
// count) of the polygon's untraversable cells (rows5: 5 doubles x g.rows), and the hull the host builds from them
hipError_t launch_polygon_untraversable_rows(const Geo& g, int n, const double* vertex_xy, const uint8_t* untrav, double* rows5,
                                             hipStream_t stream);
void untraversable_hull_from_rows(int rows, const double* rows5, std::vector<double>& hull_xy);

// the polygons checkPolygonalFootprintPath evaluates for a batch of paths (host side), in path order
constexpr int kMaxPathPolygonVertices = 1024;
struct PathPolygons {
  std::vector<int> vertex_offset;     // polygon p: vertices [vertex_offset[p], vertex_offset[p+1])
  std::vector<double> vertex_xy;
  std::vector<double> area;           // polygon.getArea()
  std::vector<double> area_previous;  // polygon1.getArea() of the same iteration (:574)
  std::vector<int> first, count, status;  // per path
};
void build_path_polygons(int n_paths, const int* pose_offset, const double* poses, int n_points, const double* points_xyz,
                         const unsigned char* conservative, PathPolygons& out);

// k_normals_fixup: every workgroup owns kFixTiles tiles that are fix_groups() apart (flagged tiles come in runs
// and must spread over many workgroups) and whose flags are adjacent in memory (one coalesced load).
// Up to 2048 tiles (a 1024 x 512 map) every tile has a workgroup of its own: a handful of flagged tiles queueing up in
// three workgroups was half of the chain's latency on the reference's own 100 x 133 map.
constexpr int kFixTiles = 8;
inline int fix_groups(int ntiles) { return ntiles <= 2048 ? ntiles : (ntiles + kFixTiles - 1) / kFixTiles; }

struct FastGrid {  // fix-up flag grid of a sliding-disc normals launch: 64x16 tiles of the region
  int ntx, nty, nbz;
  int frame;  // > 0: the fix-up pass also owns every cell within `frame` cells of the map border, whatever the flags and
              // the slope layer say (no launch asks for it today)
};

// te_stage.hip: whole-layer transfers through pageable caller buffers -- a ring of page-locked slots per context, chunked,
// the host-side copies on a process-wide pool of threads beside the DMA of the neighbouring chunk
struct HostStager {
  static constexpr size_t kChunk = (size_t)8 << 20, kMinBytes = (size_t)4 << 20;
  static constexpr int kSlots = 4;
  char* slot[kSlots] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev[kSlots] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_order = nullptr;
  hipStream_t stream = nullptr;
  int pool = 0;  // which of the process' copy-thread pools serves this ring (te_stage.hip)
  ~HostStager();
  void release();      // (with the context's device current)
  hipError_t ensure();
  // host -> device behind everything queued on `compute`; `compute` is made to wait for the data; returns once `host` may be reused
  hipError_t upload(void* dev, const void* host, size_t bytes, hipStream_t compute);
  // device -> host behind everything queued on `compute`; returns once `host` holds the data
  hipError_t download(void* host, const void* dev, size_t bytes, hipStream_t compute);
};

// The marching kernels of te_march5.h read kSlabGuardRows rows above and below the layers they are given (unconditional
// raw buffer loads, no bounds check: DESIGN.md).  Layers of a context's slab have that slack by its plan (te_slab.h); any other
// pointer -- a caller's own allocation handed in through a future entry point -- is checked here against the allocation
// that holds it, and the route plans send a layer without the slack to the bounds-checked generic kernels.
// (One driver query per distinct (pointer, shape); the verdicts are dropped whenever a context frees its layers.)
inline std::atomic<unsigned>& guard_cache_generation() {
  static std::atomic<unsigned> g{0};
  return g;
}
inline bool layer_has_guard_rows(const void* p, const Geo& g, size_t elem_bytes) {
  struct Entry {
    const void* p;
    int rows, cols, batch;
    unsigned gen;
    bool ok;
  };
  static thread_local Entry cache[8] = {};
  static thread_local int next = 0;
  const unsigned gen = guard_cache_generation().load(std::memory_order_acquire);
  for (const Entry& e : cache)
    if (e.p == p && e.rows == g.rows && e.cols == g.cols && e.batch == g.batch && e.gen == gen && p) return e.ok;
  bool ok = false;
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (p && hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) == hipSuccess) {
    const size_t guard = (size_t)kSlabGuardRows * (size_t)g.rows * elem_bytes;
    const size_t layer = (size_t)g.rows * (size_t)g.cols * (size_t)(g.batch > 0 ? g.batch : 1) * elem_bytes;
    const char* lo = (const char*)base;
    const char* hi = lo + size;
    ok = (size_t)((const char*)p - lo) >= guard && (const char*)p + layer <= hi && (size_t)(hi - ((const char*)p + layer)) >= guard;
  } else {
    (void)hipGetLastError();
  }
  cache[next] = Entry{p, g.rows, g.cols, g.batch, gen, ok};
  next = (next + 1) & 7;
  return ok;
}

// Compute units of the CURRENT device (hipGetDevice), cached per device; the launchers size their grids from it.
// (A function-local static of the first device's count would be a data race with one context per thread and the
// wrong capacity on a node with different devices.)
inline int device_cus() {
  static std::atomic<int> cache[64];
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) != hipSuccess) return cus;
  if (dev >= 0 && dev < 64) {
    const int v = cache[dev].load(std::memory_order_relaxed);
    if (v > 0) return v;
  }
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
  if (dev >= 0 && dev < 64) cache[dev].store(cus, std::memory_order_relaxed);
  return cus;
}

// te_kernels.hip: fills p.route from p's discs and parameters, the geometry and the current device (rebuild_tables)
void chain_route_template(const Geo& g, ChainParams& p);
// launch wrappers (te_kernels.hip); all asynchronous on `stream`.  hipErrorInvalidValue: a planned route without its
// instantiation, which the shim reports as an internal routing error
hipError_t launch_filter(const Geo& g, const ChainParams& p, const Layers& L, int filter, unsigned flags,
                         hipStream_t stream);
hipError_t launch_chain(const Geo& g, const ChainParams& p, const Layers& L, const Region& r, unsigned flags,
                        hipStream_t stream);
// ptab: [n_spiral] packed spiral entries (fp_pack); clip_table: build_clip_table(fp_disc, reach)
// trav_cap: upper bound of the finite traversability values if the layer was written by the chain, else < 0
// region (nullptr: all maps, all cells): the cells whose scores changed; the mask is recomputed within 3 cells of them
// and the footprint within the footprint's reach of those (a footprint shape only the general kernel serves: on every cell).
// face_flags: the face flags of the elevation layer (te_face_flags.h: "a vertical face within 2 cells" per 64 x 4 cells, built at
// upload) if they describe it now, else nullptr -- unknown, or TE_OPT_FACE_FLAGS = 0: every tile of k_fp_mask stages its step check
// The sum kernels are chosen by plan_fp_route (te_fp_route.h); a planned route without its instantiation is an error.
hipError_t launch_footprint(const Geo& g, const FootprintParams& p, const Layers& L, const uint8_t* face_flags, const unsigned* ptab,
                            const int* clip_table, bool write_memo, const ChainParams* combine, double trav_cap, hipStream_t stream,
                            const Region* region = nullptr);
// te_footprint_any.hip: the sum of the circular footprint pass at any reach (the mask kernel has run); rf: the output
// cells of map rf->map (nullptr: every cell of every map)
hipError_t launch_footprint_any(const Geo& g, const FootprintParams& p, const Layers& L, const Region* rf, hipStream_t s);
int chain_max_reach(const ChainParams& p);
// the flag grid of Layers::untrav_flags: one byte per 64 x 4 cells of every map
inline int untrav_flag_ntx(int rows) { return (rows + 63) / 64; }
inline int untrav_flag_nfy(int cols) { return (cols + 3) / 4; }
inline size_t untrav_flag_bytes(int rows, int cols, int batch) { return (size_t)untrav_flag_ntx(rows) * (size_t)untrav_flag_nfy(cols) * (size_t)batch; }
// te_paths.hip: checkCircularFootprintPath for a batch of paths on the (complete) footprint layer of one map;
// robot_slope: the layer checkInclination reads (nullptr: footprint/check_robot_inclination off)
hipError_t launch_check_circular_paths(const Geo& g, const float* footprint, double fp_default, const float* robot_slope,
                                       int n_paths, const int* pose_offset, const double* pose_xy, unsigned char* is_safe,
                                       double* traversability, int* status, hipStream_t stream);
// batched checkInclination(start, end): segment k = start_end_xy[4k .. 4k+4)
hipError_t launch_check_inclination(const Geo& g, const float* robot_slope, int n, const double* start_end_xy,
                                    unsigned char* ok, int* status, hipStream_t stream);

// te_path_discs.hip: circular path checks at each path's own radius, evaluated on demand at the visited centres
struct PathDiscClass {  // one radius class of a request
  const int4* spiral;   // FpEntry [n_spiral] of circle(radius + offset), SpiralIterator order, clipped to the map (te_fp_table.h)
  int n_spiral, pad;
  double rmin, rmax, r2;  // radius, radius + offset, (radius + offset)^2
};
enum { kPdDiscs = 0, kPdOverflow = 1, kPdVisits = 2, kPdCounters = 4 };
struct PathDiscScratch {  // the memo of one call: sized by its number of visits (te_path_visit.h: table_entries)
  uint64_t* keys;      // [mask + 1] open-addressing table of pack_key(class, cell); kEmptyKey: free
  float* vals;         // [mask + 1] the disc's value beside its key
  unsigned* list;      // [list_cap] slots in the order of their first insertion: the discs to evaluate
  unsigned* counters;  // [kPdCounters]: discs listed, "table or list full", centres visited
  uint64_t mask;
  unsigned list_cap;
};
// the three phases (visit, discs, paths) on `stream`; trav / untrav / robot_slope: the layers of the map the paths are on
hipError_t launch_path_discs(const Geo& g, const PathDiscScratch& s, const PathDiscClass* classes, const float* trav, const uint8_t* untrav,
                             double fp_default, const float* robot_slope, int n_paths, const int* pose_offset, const double* pose_xy,
                             const int* path_class, unsigned char* is_safe, double* traversability, int* status, hipStream_t stream);
// te_footprint.hip: the isTraversableForFilters mask of every cell of every map (Layers::untrav, untrav_flags) and nothing
// else: no memo layers, no footprint layer; combine: also the weighted sum a whole-map chain left to the mask kernel;
// face_flags: as for launch_footprint
hipError_t launch_footprint_mask(const Geo& g, const FootprintParams& p, const Layers& L, const uint8_t* face_flags, const ChainParams* combine,
                                 hipStream_t stream);

// te_filter_any.hip: the filters for the discs marked Disc::any (the other disc of a normals stage may be either kind)
namespace any {
struct NormalsJob {  // k_normals' arguments
  Disc dn, dr;
  int same_disc, axis, rank_rule;
  int combine;        // also write the traversability layer (reads the step layer)
  int given_normals;  // RoughnessFilter alone: surface_normal_{x,y,z} are input layers
  double slope_crit, rough_crit;
  float w_scale, w_slope, w_step, w_rough;
};
hipError_t step_height(const Geo& g, const Disc& d, const float* elev, float* sh, const Region& r, hipStream_t s);
hipError_t step_score(const Geo& g, const Disc& d, double crit, int ncrit, const float* sh, float* out, const Region& r, hipStream_t s);
// nx, ny, nz: the normals to keep (nullptr: none); with given_normals the input normals
hipError_t normals(const Geo& g, const NormalsJob& a, const Layers& L, float* nx, float* ny, float* nz, const Region& r, hipStream_t s);
}  // namespace any

// The shape-specialised kernels of the filter chain, each the launcher of ONE route plan_chain_route (te_chain_route.h)
// names: they build their argument block and launch.  hipErrorInvalidValue: a planned route without its instantiation
// (an internal routing error, never a slower kernel).
namespace fast {
inline FastGrid fast_grid(const Geo& g, const Region& r) {  // the fix-up flag grid of region r
  return FastGrid{(r.i1 - r.i0 + 63) / 64, (r.j1 - r.j0 + 15) / 16, r.map >= 0 ? 1 : g.batch, 0};
}
// te_fast_step.hip: k_step_small on the disc's window (the centre alone, or a tie radius of one or two cells)
hipError_t step_height_small(const Disc& d, const Geo& g, const float* elev, float* sh, const Region& r, hipStream_t s);
hipError_t step_score_small(const Disc& d, const Geo& g, double crit, int ncrit, const float* sh, float* out, const Region& r, hipStream_t s);
// te_step5.hip: the marching kernels on shape Q (RAW -- second output pointer set -- behind the two *_ties below)
hipError_t step_height5(int Q, const Geo& g, const float* elev, float* sh, float* sh_min, const Region& r, hipStream_t s);
hipError_t step_score5(int Q, const Geo& g, double crit, int ncrit, const float* sh, float* out, float* out_count, const Region& r, hipStream_t s);
// ... at a tie radius (whole-cell radii of 3 .. 10 cells): the RAW march on q, the shape without its circle, then the
// accepted circle cells folded in per cell; scratch: one float per cell of the layer (Layers::tie_scratch)
hipError_t step_height_ties(const Disc& d, int q, const Geo& g, const float* elev, float* sh, float* scratch, const Region& r, hipStream_t s);
hipError_t step_score_ties(const Disc& d, int q, const Geo& g, double crit, int ncrit, const float* sh, float* out, float* scratch,
                           const Region& r, hipStream_t s);
// te_slide_normals.hip: k_normals_slide for the tie-free disc d (sii: sum of di^2 over it), shape or radius form; given:
// RoughnessFilter alone with the normals of the layers; combine: the traversability layer is written too (the step layer
// must be complete)
hipError_t normals_slide(const Geo& g, const ChainParams& p, const Layers& L, const Disc& d, int sii, bool shape_form, bool given,
                         bool keep_normals, bool combine, const Region& r, int* block_flags, hipStream_t s);
// te_normals3.hip: k_normals3 / k_normals3s, the cells whose disc lies inside the map; march, shape and strips from rt
hipError_t normals3(const Geo& g, const ChainParams& p, const Layers& L, const ChainRoute& rt, const DiscSummary& ds, const Region& r,
                    int* block_flags, hipStream_t s);
// te_normals_small.hip: discs that reach at most two cells, one cell per thread, no fix-up pass behind it
// write_step: both step windows hold one cell -- the step score is 1 (valid) / NaN and this kernel writes the layer; combine:
// ... and the weighted sum (the step layer must be complete, or written here)
hipError_t normals_small(const Geo& g, const ChainParams& p, const Layers& L, bool keep_normals, bool cross, const Region& r, hipStream_t s,
                         bool write_step, bool combine);
// ... and the whole chain of a small whole-map launch in one kernel (k_chain_window)
hipError_t chain_window(const Geo& g, const ChainParams& p, const Layers& L, bool keep_normals, const Region& r, bool combine, hipStream_t s);
// te_normals_raster.hip: NormalVectorsFilter's raster method on every cell of every map: the three normal layers, and with
// `slope` (the chain form; nullptr: the normals alone) traversability_slope
hipError_t normals_raster(const Geo& g, int axis, double slope_crit, const float* elev, float* nx, float* ny, float* nz, float* slope,
                          hipStream_t s);
int normals_fast_max_blocks(const Geo& g);
size_t normals_hole_queue_bytes();  // te_normals3.hip: scratch of the sparse-hole march for one device (any map, any batch)
// The sum kernels of the circular footprint pass, each on the route plan_fp_route chose for it (false: the shape is not
// instantiated).  region: the output cells to compute (whole block columns and the rows [j0, j1) of map `map`); nullptr:
// every map, every cell.  te_footprint5.hip: the scatter-form sum on fixed point (tie-free discs up to 15 cells);
// te_footprint4.hip: the sliding sum on fixed point (whole-cell tie radii); te_footprint3.hip: the sliding sum in double.
bool footprint_slide5(const Geo& g, const FootprintParams& p, const Layers& L, const int* clip_table, const FpRoute& r, hipStream_t s,
                      const Region* region);
bool footprint_slide4(const Geo& g, const FootprintParams& p, const Layers& L, const int* clip_table, const FpRoute& r, hipStream_t s,
                      const Region* region);
bool footprint_slide3(const Geo& g, const FootprintParams& p, const Layers& L, const unsigned* ptab, const int* clip_table, hipStream_t s,
                      const Region* region);
constexpr int kClipInts = 6 * (2 * kMaxRadiusCells + 1) * (2 * kMaxRadiusCells + 1);  // one clip table of the normals disc; for a tie radius the
                                                                                      // table of the disc with its circle follows, then the packed offsets
constexpr int kFpClipInts = 6 * 41 * 41;  // one clip table of the footprint disc (reach <= 20); a second one follows it for a tie
                                           // radius: the disc with the cells on its circle (k_fp_slide4<Q, true>)
// the second half of a fixed-point pass (FpRoute::blocked): the listed cells, after every launch of the pass
void footprint_blocked4(const Geo& g, const FootprintParams& p, const Layers& L, const unsigned* ptab, hipStream_t s);
}  // namespace fast

}  // namespace te
