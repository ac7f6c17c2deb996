// te_shim.hip -- C-ABI of libtravgpu.so (declared in include/travgpu.h).
//
// Owns the device-resident elevation/output layers of a batch of maps and launches the HIP chain.
// No CPU fallback of any kind: without a gfx950 device te_create() fails with TE_ERR_NO_DEVICE.
#include "te_ctx.h"
#include "te_expr_launch.h"
#include "te_fp_table.h"
#include "te_hole_routing.h"

using namespace te;
using namespace te::shim;

namespace te {
namespace shim {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

// build_disc (te_disc.h) for the window `what`, its refusals as the error of the entry point
int named_disc(double radius, double res, Disc* d, const char* what) {
  const DiscStatus st = build_disc(radius, res, d);
  if (st == kDiscTooLarge)
    return fail(TE_ERR_UNSUPPORTED, "%s radius %.6g m is %.2f cells; this build supports up to %d", what, radius, radius / res, kMaxRadiusCells);
  return st == kDiscTooManyTies ? fail(TE_ERR_UNSUPPORTED, "%s radius: too many tie offsets", what) : TE_OK;
}

// A filter disc: build_disc's fixed arrays, or under TE_OPT_FILTER_ANY_RADIUS the table of any radius (te_disc_table.h) --
// option 1 for the discs build_disc refuses, option 2 for every disc.  The device table is set by upload_any_discs.
int filter_disc(te_ctx* c, double radius, Disc* d, DiscTable* t, const char* what) {
  *t = DiscTable();
  if (c->opt_filter_any != 2) {
    char before[sizeof(g_err)];
    memcpy(before, g_err, sizeof(before));
    const int rc = named_disc(radius, c->geo.res, d, what);
    if (rc == TE_OK || c->opt_filter_any == 0) return rc;
    memcpy(g_err, before, sizeof(before));  // (the refusal is not an error under option 1)
  }
  build_disc_table(radius, c->geo.res, t);
  memset(d, 0, sizeof(*d));
  d->R = t->R;
  for (int b = 0; b <= kMaxRadiusCells; ++b) d->hw[b] = -1;
  d->n_ties = t->n_ties();
  d->r2 = t->r2;
  d->reach = t->reach;
  d->npoints = t->npoints < 0x7fffffff ? (int)t->npoints : 0x7fffffff;
  d->Q = -1;
  d->any = 1;
  d->any_hw0 = t->R >= 0 ? t->hw[0] : -1;
  d->tab = nullptr;
  return TE_OK;
}

// the tables of the discs marked Disc::any on the device, in one buffer (grown when a larger one is needed)
int upload_any_discs(te_ctx* c) {
  Disc* ds[4] = {&c->cp.normals, &c->cp.rough, &c->cp.step1, &c->cp.step2};
  std::vector<int32_t> ints;
  size_t off[4] = {0, 0, 0, 0};
  for (int k = 0; k < 4; ++k) {
    if (!ds[k]->any) continue;
    off[k] = ints.size();
    ints.insert(ints.end(), c->fa_host[k].hw.begin(), c->fa_host[k].hw.end());
    ints.insert(ints.end(), c->fa_host[k].ties.begin(), c->fa_host[k].ties.end());
    ints.push_back(0);  // (an empty disc still gets an address of its own)
  }
  if (ints.empty()) return TE_OK;
  const size_t bytes = ints.size() * sizeof(int32_t);
  HIP_TRY(hipSetDevice(c->device));
  if (c->cmem.fa_tab.reserve(bytes, c->stream) != hipSuccess)
    return fail(TE_ERR_UNSUPPORTED, "filter discs of any radius: their tables (%zu bytes) do not fit in device memory", bytes);
  HIP_TRY(hipMemcpyAsync(c->cmem.fa_tab.p, ints.data(), bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int k = 0; k < 4; ++k)  // (every Disc::tab is derived again: the buffer may have moved)
    if (ds[k]->any) ds[k]->tab = c->cmem.fa_tab.as<const int>() + off[k];
  return TE_OK;
}

}  // namespace shim
}  // namespace te


// The upload's pass over the whole elevation layer: one kernel, one wait.
// Invalid (non-finite) cells: out[0] their number; out[1] the number of RUNS of them in memory order (an invalid cell whose
// predecessor is valid, or that is the layer's first).  The two pick the march k_normals3 uses for strips with invalid cells
// and its strip height: scattered cells (runs of one) against unobserved regions (runs as long as the regions are wide),
// te_normals3.hip.
// Face flags (te_face_flags.h): one byte per 64 x 4 cells, 1 iff some cell within 2 cells of the granule lies more than
// crit_step above the lowest cell of its 3x3 block.  A wavefront owns one flag column (64 cells along i) over 32 columns of
// the map (8 granules) and marches down j through them and a halo of 3 (2 cells of dilation + 1 of the 3x3 block; NaN
// outside the map), straight from global memory: a lane loads its cell and the two beside it, the minimum of the three
// slides over three steps in registers, and the lanes do the same for the two cells either side of the 64.  A step's
// verdict is one bit of a wave-uniform word; a granule's flag ORs its own 4 steps and 2 either side: the dilation is done
// here, the mask kernel reads only its own bytes.  The counts come from the same loads.
namespace {
constexpr int kCfX = 64, kCfY = 32, kCfH = te::kFaceDilate + 1, kCfT = kCfY + 2 * kCfH, kCfWaves = 4, kCfG = 10;
static_assert(kCfX == te::kFaceGranI && kCfY % te::kFaceGranJ == 0 && kCfT <= 64 && kCfY / te::kFaceGranJ <= 64, "k_count_invalid: tile shape");
}  // namespace
__global__ __launch_bounds__(64 * kCfWaves) void k_count_invalid(const float* __restrict__ v, int rows, int cols, double crit_step,
                                                                 uint8_t* __restrict__ flags, unsigned long long* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ti = (int)blockIdx.x * kCfWaves + wave;
  if (ti >= te::face_flag_ntx(rows)) return;  // (whole wavefronts; the kernel has no barrier)
  const int map = blockIdx.z, i0 = ti * kCfX, j0 = (int)blockIdx.y * kCfY;
  const size_t mo = (size_t)map * (size_t)rows * (size_t)cols;
  const float nan = __builtin_nanf("");
  // Every load is unconditional: a column's base is wave-uniform, a lane's offsets are fixed before the loop, and a neighbour
  // outside the map reads the cell itself, which leaves the minimum as it is.  No branch and no address arithmetic stands
  // between the loads of a group of steps.
  const int i = i0 + lane, ic = i < rows ? i : rows - 1;
  const bool own = i < rows, has_up = i > 0;
  const int o_prev = ic - 1, o_prev0 = ic > 0 ? ic - 1 : 0, o_next = ic + 1 < rows ? ic + 1 : ic;
  // the two cells either side of the 64: lanes 4 q + 0, 1 take i0 - 2, i0 - 1, lanes 4 q + 2, 3 take i0 + 64, i0 + 65 (every q the same)
  const int xl = lane & 3;
  const int ix = xl < te::kFaceDilate ? i0 - te::kFaceDilate + xl : i0 + kCfX + xl - te::kFaceDilate;
  const bool xin = ix >= 0 && ix < rows;
  const int ixc = ix < 0 ? 0 : (ix < rows ? ix : rows - 1);
  const int ox_prev = ixc > 0 ? ixc - 1 : 0, ox_next = ixc + 1 < rows ? ixc + 1 : ixc;
  auto mn = [](float a, float b) { return __builtin_fminf(a, b); };  // (ignores NaN like te::face_min; the sign of a zero does not reach the test)
  unsigned cnt = 0, runs = 0;
  unsigned long long step_any = 0ull;  // bit r: some cell of step r (map column j0 - kCfH + r) has the face test true
  float a0 = nan, a1 = nan, e1 = nan, x0 = nan, x1 = nan, ex1 = nan;  // minima of the two steps before, and the cells of the one before
  // kCfG steps at a time: all their loads first, into registers, then the arithmetic (a step's loads wait for nothing)
#pragma unroll
  for (int rb = 0; rb < kCfT; rb += kCfG) {
    float prev[kCfG], mid[kCfG], next[kCfG], xprev[kCfG], xmid[kCfG], xnext[kCfG];
#pragma unroll
    for (int q = 0; q < kCfG; ++q) {
      if (rb + q >= kCfT) continue;
      const int j = j0 - kCfH + rb + q;
      const size_t col = mo + (size_t)(j < 0 ? 0 : (j < cols ? j : cols - 1)) * rows;
      const float* __restrict__ cp = v + col;
      // the predecessor in memory: the cell above, or the last cell of the previous column / map (none before the layer's first)
      prev[q] = cp[col == 0 ? o_prev0 : o_prev], mid[q] = cp[ic], next[q] = cp[o_next];
      xprev[q] = cp[ox_prev], xmid[q] = cp[ixc], xnext[q] = cp[ox_next];
    }
#pragma unroll
    for (int q = 0; q < kCfG; ++q) {
      const int r = rb + q;
      if (r >= kCfT) continue;
      const int j = j0 - kCfH + r;
      const bool jin = j >= 0 && j < cols;  // (uniform)
      const bool in = jin && own, inx = jin && xin;
      const float e2 = in ? mid[q] : nan, ex2 = inx ? xmid[q] : nan;
      const float a2 = in ? mn(mn(has_up ? prev[q] : mid[q], mid[q]), next[q]) : nan;
      const float x2 = inx ? mn(mn(xprev[q], xmid[q]), xnext[q]) : nan;
      if (r >= kCfH && r < kCfH + kCfY) {  // the two counts: every cell of the layer belongs to exactly one wavefront
        const bool bad = in && !__builtin_isfinite(mid[q]);
        const bool first = map == 0 && j == 0 && i == 0;
        cnt += bad ? 1u : 0u;
        runs += (bad && (first || __builtin_isfinite(prev[q]))) ? 1u : 0u;
      }
      if (r >= 2) {  // step r - 1 has its three minima (a cell outside the map is NaN and never hits)
        const bool hit = te::face_hit(mn(mn(a0, a1), a2), e1, crit_step) || te::face_hit(mn(mn(x0, x1), x2), ex1, crit_step);
        if (__ballot(hit) != 0ull) step_any |= 1ull << (r - 1);
      }
      a0 = a1, a1 = a2, e1 = e2;
      x0 = x1, x1 = x2, ex1 = ex2;
    }
  }
  for (int d = 32; d >= 1; d >>= 1) {
    cnt += __shfl_xor((int)cnt, d);
    runs += __shfl_xor((int)runs, d);
  }
  if (lane == 0 && cnt) {
    atomicAdd(out, (unsigned long long)cnt);
    if (runs) atomicAdd(out + 1, (unsigned long long)runs);
  }
  if (flags != nullptr && lane < kCfY / te::kFaceGranJ) {  // granule `lane`: its own steps kCfH + 4 lane .. + 3, and kFaceDilate either side
    const int fj = j0 / te::kFaceGranJ + lane;
    if (fj < te::face_flag_nfy(cols)) {
      const unsigned long long span = (1ull << (te::kFaceGranJ + 2 * te::kFaceDilate)) - 1ull;
      const bool any = ((step_any >> (kCfH - te::kFaceDilate + te::kFaceGranJ * lane)) & span) != 0ull;
      flags[((size_t)map * (size_t)te::face_flag_nfy(cols) + (size_t)fj) * (size_t)te::face_flag_ntx(rows) + (size_t)ti] = any ? 1 : 0;
    }
  }
}


namespace te {
namespace shim {
// joins a running prefetch (caller holds c->mu); its result stays in c->prefetch_rc until te_wait_prefetch reports it
void finish_prefetch_locked(te_ctx* c) {
  {
    std::unique_lock<std::mutex> pl(c->pf_mu);
    if (!c->prefetch_running && !c->prefetch_mask) return;
    c->pf_cv.wait(pl, [c] { return !c->prefetch_running; });
  }
  const unsigned mask = c->prefetch_mask;
  c->prefetch_mask = 0;
  c->prefetch_elev = false;
  const bool ok = c->prefetch_rc.load() == TE_OK;
  c->st.prefetch_joined(mask, ok);
  // an arrived elevation: the invalid cells are counted like te_upload_elevation counts them (the count picks the normals
  // kernel's march and strip height); a failure leaves the count unknown, which every kernel serves
  if (ok && (mask & bit(TE_LAYER_ELEVATION)) && (hipSetDevice(c->device) != hipSuccess || count_invalid_elevation(c) != TE_OK)) {
    (void)hipGetLastError();
    c->st.count_unknown();
  }
}
// layers TE_FILTER_* reads and writes (travgpu.h: TE_FILTER_* table)
unsigned filter_layers(int filter) {
  const unsigned normals = bit(TE_LAYER_NORMAL_X) | bit(TE_LAYER_NORMAL_Y) | bit(TE_LAYER_NORMAL_Z);
  switch (filter) {
    case TE_FILTER_SLOPE: return bit(TE_LAYER_NORMAL_Z) | bit(TE_LAYER_SLOPE);
    case TE_FILTER_STEP: return bit(TE_LAYER_ELEVATION) | bit(TE_LAYER_STEP);
    case TE_FILTER_ROUGHNESS: return bit(TE_LAYER_ELEVATION) | normals | bit(TE_LAYER_ROUGHNESS);
    case TE_FILTER_COMBINE: return bit(TE_LAYER_SLOPE) | bit(TE_LAYER_STEP) | bit(TE_LAYER_ROUGHNESS) | bit(TE_LAYER_TRAVERSABILITY);
    case TE_FILTER_NORMALS: return bit(TE_LAYER_ELEVATION) | normals | bit(TE_LAYER_SLOPE) | bit(TE_LAYER_ROUGHNESS);
    default: return ~0u;
  }
}
}  // namespace shim
}  // namespace te

namespace te {
namespace shim {

// counts the invalid cells of the whole elevation layer on the context's stream, builds the layer's face flags for the
// fp_critical_step held (te_face_flags.h) and waits for the result
int count_invalid_elevation(te_ctx* c) {
  c->st.count_unknown();
  HIP_TRY(c->cmem.count.once(2 * sizeof(unsigned long long)));
  unsigned long long* const d_count = c->cmem.count.as<unsigned long long>();
  HIP_TRY(hipMemsetAsync(d_count, 0, 2 * sizeof(unsigned long long), c->stream));
  const bool with_flags = c->face_flags != nullptr;
  const double crit = c->params.fp_critical_step;
  const dim3 grid((unsigned)((face_flag_ntx(c->geo.rows) + kCfWaves - 1) / kCfWaves), (unsigned)((c->geo.cols + kCfY - 1) / kCfY), (unsigned)c->geo.batch);
  if (grid.y > 65535u || grid.z > 65535u) return fail(TE_ERR_UNSUPPORTED, "elevation layer of %d columns x %d maps: too many for one pass", c->geo.cols, c->geo.batch);
  hipLaunchKernelGGL(k_count_invalid, grid, dim3(64 * kCfWaves), 0, c->stream, c->L.elev, c->geo.rows, c->geo.cols, crit, c->face_flags, d_count);
  HIP_TRY(hipGetLastError());
  unsigned long long h[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(h, d_count, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->st.elevation_counted((long long)h[0], (long long)h[1], with_flags ? crit : __builtin_nan(""));
  return TE_OK;
}

// the face flags a mask launch may read: built for the elevation that is resident and for the critical step of the footprint
// parameters in force (NaN -- unknown -- compares false)
const uint8_t* usable_face_flags(const te_ctx* c) {
  return (c->opt_face_flags && c->face_flags && c->st.face_flags_for(c->fp.crit_step, c->params.fp_critical_step)) ? c->face_flags : nullptr;
}

// few invalid cells, scattered: at most 2 per mille (0.1 % speckle: the sparse march is 1.4x faster than the dense one,
// at 1 % 1.4x slower; MI355X, 4096^2, R = 9).  Unknown counts take the dense march, whose cost does not depend on the map.
// (A map without invalid cells takes the dense kernel too: its clean march is the same code, and a tile with invalid
// cells uploaded later -- tiles are not counted -- is then in safe hands.)
// Which march serves the invalid cells of the resident elevation layer: te_hole_routing.h (plain functions of the upload's
// two counts, shared with the CPU test); the lab switches stay here.
HoleCounts hole_counts(const te_ctx* c) { return c->st.hole_counts((long long)c->layer_elems); }
bool clustered_holes(const te_ctx* c) { return holes_clustered(hole_counts(c)); }
bool sparse_holes(const te_ctx* c) {
  static const int force = lab_int("TE_N3_HOLES", 0);  // measurement aid: 1 sparse, 2 dense
  if (force == 1 || force == 2) return force == 1;
  return holes_sparse(hole_counts(c));
}
bool skip_clean_march(const te_ctx* c) {
#ifdef TE_NO_SKIP_CLEAN  // (A/B builds only)
  return false;
#endif
  return sparse_holes(c) && holes_skip_clean_march(hole_counts(c));
}
bool short_strips(const te_ctx* c) {
  static const int force = lab_int("TE_N3_SHORT_STRIPS", -1);  // measurement aid: 0 never, 1 whenever invalid cells were counted
  if (force >= 0) return force == 1 && c->st.invalid_cells() > 0 && !sparse_holes(c);
  return clustered_holes(c) && !sparse_holes(c);
}

// the sparse march's queues; false (and the dense kernel) if the allocation fails
bool ensure_hole_queue(te_ctx* c) {
  if (c->cmem.hole_queue.p) return true;
  return hipSetDevice(c->device) == hipSuccess && c->cmem.hole_queue.once(fast::normals_hole_queue_bytes()) == hipSuccess;
}

// the step filter's scratch layer at a tie radius (te_fast_step.hip); without it the generic kernels serve
void ensure_tie_scratch(te_ctx* c) {
  if (c->lmem.tie_scratch.p || !c->tables_ready || c->layer_elems == 0) return;
  if ((c->cp.step1.n_ties == 0 || c->cp.step1.any) && (c->cp.step2.n_ties == 0 || c->cp.step2.any)) return;
  if (hipSetDevice(c->device) == hipSuccess) (void)c->lmem.tie_scratch.once(c->layer_elems * sizeof(float));
}

// What picks the kernel variants of a whole-map launch beside its flags: the march k_normals3 runs, from the upload's count,
// and whether the mask kernel is given the face flags.  A captured launch bakes them in, so they are decided in ONE place:
// set_launch_hints hands them to the kernels and run_whole_locked packs its graph key from the same struct.
struct LaunchHints {
  bool sparse_holes, no_holes, skip_clean, short_strips, face_flags;
  // the upper bits of the graph key, above the TE_RUN_* bits (the face flags matter to a launch with the footprint pass)
  unsigned key_bits(unsigned flags) const {
    return (sparse_holes ? 0x80000000u : 0u) | (no_holes ? 0x40000000u : 0u) | (skip_clean ? 0x20000000u : 0u) | (short_strips ? 0x10000000u : 0u) |
           (((flags & TE_RUN_FOOTPRINT) && face_flags) ? 0x08000000u : 0u);
  }
};
// ... with the two scratch buffers the variants need, allocated on first need and outside any capture (run_whole_locked asks
// before it captures); a failed allocation leaves the pointer null and the kernels that need none serve
LaunchHints launch_hints(te_ctx* c) {
  LaunchHints h;
  h.sparse_holes = sparse_holes(c) && ensure_hole_queue(c);
  h.no_holes = c->st.invalid_cells() == 0;
  h.skip_clean = h.sparse_holes && skip_clean_march(c);
  h.short_strips = short_strips(c);
  h.face_flags = usable_face_flags(c) != nullptr;
  ensure_tie_scratch(c);
  return h;
}

// What a launch of the filters takes from the context beside its parameters: the hints, TE_OPT_NORMALS_RANK_RULE, and the
// pointers derived from the two scratch buffers
void set_launch_hints(te_ctx* c) {
  const LaunchHints h = launch_hints(c);
  c->L.sparse_holes = h.sparse_holes ? 1 : 0;
  c->L.no_holes = h.no_holes ? 1 : 0;
  c->L.skip_clean = h.skip_clean ? 1 : 0;
  c->L.short_strips = h.short_strips ? 1 : 0;
  c->L.hole_queue = c->cmem.hole_queue.as<char>();
  c->L.tie_scratch = c->lmem.tie_scratch.as<float>();
  c->cp.rank_rule = c->opt_rank_rule;
  c->cp.raster = c->opt_normals_raster;
}

// TE_OPT_NORMALS_RANK_RULE decides on the rank of an exactly planar disc; on a normals disc above 32 cells the moment form's
// pivot test and the oracle's (centred points, 3 eps) disagree on rounding noise, so the combination is refused
// (The raster method has no disc and no rank: the rule has no effect there.)
int refuse_rank_rule(te_ctx* c) {
  if (c->opt_rank_rule && !c->opt_normals_raster && c->cp.normals.any)
    return fail(TE_ERR_UNSUPPORTED, "TE_OPT_NORMALS_RANK_RULE is not supported with a normals disc of the route of any radius (%d cells)",
                c->cp.normals.R);
  return TE_OK;
}

void drop_graph(te_ctx* c) {
  for (int k = 0; k < te_ctx::kGraphs; ++k) {
    if (c->graph_exec[k]) (void)hipGraphExecDestroy(c->graph_exec[k]);
    c->graph_exec[k] = nullptr;
  }
}

// the pointers into the buffers of the route of any reach (lmem.fpa): cleared wherever those are released
void clear_fp_any_ptrs(te_ctx* c) {
  c->fp.any_spiral = nullptr;
  c->fp.any_ints = nullptr;
  c->fp.any_psum = nullptr;
  c->fp.any_pcnt = nullptr;
}
void release_fp_any(te_ctx* c) {
  c->lmem.fpa = te_ctx::LayerMem::FpAny();
  clear_fp_any_ptrs(c);
}

// (device memory for the route of any reach: the only way its tables can fail).  The message names what sent the pass
// there: the reach, the option, or -- up to 20 cells -- a traversability layer without the bound the double kernels need.
static int fp_any_alloc(te_ctx* c, DevBuf& buf, size_t bytes, const char* what) {
  if (buf.reserve(bytes, c->stream) == hipSuccess) return TE_OK;
  if (c->fp.reach > 20)
    return fail(TE_ERR_UNSUPPORTED, "footprint radius %.3g m is %d cells: its %s (%zu bytes) do not fit in device memory", c->fp.rmax,
                c->fp.reach, what, bytes);
  if (c->opt_fp_any)
    return fail(TE_ERR_UNSUPPORTED, "footprint with TE_OPT_FP_ANY_REACH: the %s of the route of any reach (%zu bytes) do not fit in device memory",
                what, bytes);
  return fail(TE_ERR_UNSUPPORTED,
              "footprint: the traversability layer has no known bound (written from outside, or a large or negative weight or "
              "default) and is summed on the route of any reach, whose %s (%zu bytes) do not fit in device memory",
              what, bytes);
}

// The tables of the route of any reach (te_footprint_any.hip) on the device: run half-widths, those of the inner disc (the
// rings within radiusMin that the SpiralIterator takes whole, fp_inner_rings of te_fp_table.h), the tie offsets, the spiral; and
// the prefix-sum scratch of the maps.  Allocated here and never inside a launch (whole-map launches are captured).
int build_fp_any_tables(te_ctx* c, const FpTable& t) {
  FootprintParams& f = c->fp;
  const Geo& g = c->geo;
  std::vector<int32_t> ints(t.hw.begin(), t.hw.end());
  f.any_R = t.R;
  if (!fp_inner_rings(t, footprint_inner_q(g.res, f.rmin, f.rmax), g.rows, g.cols, &ints, &f.any_inner_R, &f.any_k_inner))
    return fail(TE_ERR_UNSUPPORTED, "footprint: the inner rings are not a prefix of the spiral");
  ints.insert(ints.end(), t.ties.begin(), t.ties.end());
  f.any_n_ties = (int)t.ties.size() / 2;
  f.any_n_spiral = (int)t.spiral.size();
  while (ints.size() % 4) ints.push_back(0);  // (the spiral behind them 16-byte aligned)
  const size_t ib = ints.size() * sizeof(int32_t), sb = t.spiral.size() * sizeof(FpEntry);
  HIP_TRY(hipSetDevice(c->device));
  int rc;
  clear_fp_any_ptrs(c);  // (a failure leaves no pointer into a buffer that was freed on the way)
  DevBuf& tab = c->lmem.fpa.tab;
  DevBuf& prefix = c->lmem.fpa.prefix;
  if ((rc = fp_any_alloc(c, tab, ib + sb, "tables"))) return rc;
  const size_t cells = (size_t)g.batch * g.cols * (size_t)(g.rows + 1);
  if ((rc = fp_any_alloc(c, prefix, cells * (sizeof(double) + sizeof(unsigned)), "prefix sums"))) return rc;
  HIP_TRY(hipMemcpyAsync(tab.p, ints.data(), ib, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(tab.as<char>() + ib, t.spiral.data(), sb, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  f.any_ints = tab.as<const int>();
  f.any_spiral = (const int*)(tab.as<const char>() + ib);
  f.any_psum = prefix.as<double>();
  f.any_pcnt = (unsigned*)(prefix.as<char>() + cells * sizeof(double));
  return TE_OK;
}

// A footprint pass over a layer bounded by trav_cap (< 0: no bound known) is about to be launched: if the plan will send it
// to the route of any reach for want of a bound (te_fp_route.h), that route's tables and prefix sums exist afterwards.
// Never allocates for a pass right behind a whole-map chain (the only captured one): its bound is the weights' own, and
// rebuild_footprint_tables_impl has built the tables for it.
int ensure_fp_any(te_ctx* c, double trav_cap) {
  const FootprintParams& f = c->fp;
  if (f.any || f.any_psum) return TE_OK;
  if (fast::fp_packed_ok((double)f.fp_disc.npoints + (double)f.fp_disc.n_ties, trav_cap, f.def)) return TE_OK;
  FpTable any;
  build_fp_table(f.rmax, c->geo.res, c->geo.rows, c->geo.cols, &any);
  return build_fp_any_tables(c, any);
}

// Discs of the three footprint checks, SpiralIterator order and clip table of the circular footprint pass.  A failure is
// recorded (fp_tables_rc / fp_tables_err) and reported by the entry points that need the footprint, not by the chain.
int rebuild_footprint_tables_impl(te_ctx* c) {
  const te_params& p = c->params;
  const double res = c->geo.res;
  int rc;
  // ---- circular footprint: discs of the three checks, spiral order, clip table ----------------------
  {
    FootprintParams& f = c->fp;
    if ((rc = named_disc(3.0 * res, res, &f.slope_disc, "footprint slope window"))) return rc;   // TraversabilityMap.cpp:871
    if ((rc = named_disc(2.5 * res, res, &f.step_disc, "footprint step window"))) return rc;     // :798
    f.rmin = p.fp_radius;
    f.rmax = p.fp_radius + p.fp_offset;  // :312 isTraversable(center, radius + offset, ..., radius)
    f.def = p.fp_default;
    f.max_gap = p.fp_max_gap;
    f.crit_step = p.fp_critical_step;
    f.check_rough = p.fp_check_roughness;
    {
      const double wr = 3.0 * res, crit_len = p.fp_max_gap / 3.0;
      f.ncrit_slope = (int)floor(2 * wr * crit_len / pow(res, 2));    // :873
      f.ncrit_rough = (int)floor(1.5 * wr * crit_len / pow(res, 2));  // :901
    }
    // the spiral of any reach, clipped to the map (te_fp_table.h): its reach picks the route.  Above 20 cells the route of
    // any reach serves the pass, and fp_disc and the tables of the shape-specialised kernels are not built.
    FpTable any;
    build_fp_table(f.rmax, res, c->geo.rows, c->geo.cols, &any);
    f.any = (c->opt_fp_any || any.reach > 20) ? 1 : 0;
    if (any.reach > 20) {
      memset(&f.fp_disc, 0, sizeof(f.fp_disc));
      f.fp_disc.R = -1;
      f.fp_disc.r2 = f.rmax * f.rmax;
      f.reach = any.reach;
      f.n_spiral = 0;
      return build_fp_any_tables(c, any);
    }
    if ((rc = named_disc(f.rmax, res, &f.fp_disc, "footprint"))) return rc;
    const Disc& d = f.fp_disc;
    // the same spiral unclipped (the kernels clip it per centre), one packed word per entry: the kernels' spiral walks read
    // it with scalar loads, eight entries at a time
    FpTable sp;
    build_fp_table(f.rmax, res, c->geo.rows, c->geo.cols, &sp, false);
    f.n_spiral = (int)sp.spiral.size();
    f.reach = sp.reach;
    if (f.reach > 20 || f.n_spiral > kMaxSpiral)  // (a reach above 20 cells took the route of any reach above)
      return fail(TE_ERR_UNSUPPORTED, "footprint radius %.3g m is %d cells: internal routing error", f.rmax, f.reach);
    std::vector<uint32_t> packed(f.n_spiral);
    for (int k = 0; k < f.n_spiral; ++k) packed[k] = fp_pack(sp.spiral[k]);
    std::vector<int> ctab((size_t)(2 * f.reach + 1) * (2 * f.reach + 1) * 6);
    build_clip_table(d, f.reach, ctab.data());
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->cmem.spiral.once(sizeof(uint32_t) * kMaxSpiral));
    HIP_TRY(hipMemcpyAsync(c->cmem.spiral.p, packed.data(), packed.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c->cmem.fp_clip_table.once(sizeof(int) * (2 * fast::kFpClipInts + kMaxTies)));
    int* const fp_clip_table = c->cmem.fp_clip_table.as<int>();
    std::vector<int> ctab_full;
    TieCircle tc;
    if (d.n_ties) {  // the disc with the cells on its circle (fixed-point sliding sum of a tie radius, te_footprint4.hip) ...
      build_tie_circle(d, &tc);  // ... and the offsets on the circle with both parts non-zero, packed, behind it
      ctab_full.resize(ctab.size());
      build_clip_table(tc.full, f.reach, ctab_full.data());
      HIP_TRY(hipMemcpyAsync(fp_clip_table + fast::kFpClipInts, ctab_full.data(), ctab_full.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
      if (tc.n_gen) HIP_TRY(hipMemcpyAsync(fp_clip_table + 2 * fast::kFpClipInts, tc.gen, tc.n_gen * sizeof(int), hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(hipMemcpyAsync(fp_clip_table, ctab.data(), ctab.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    // TE_OPT_FP_ANY_REACH -- or a layer of the chain's own that lacks the bound the double kernels need (te_fp_route.h: a
    // large or negative weight, a large default): such a pass takes the route of any reach, and a captured launch cannot
    // allocate.  A layer from outside gets the tables when a pass first meets it (ensure_fp_any).
    if (f.any || !fast::fp_packed_ok((double)d.npoints + (double)d.n_ties, weights_cap(p.w_scale, p.w_slope, p.w_step, p.w_rough), f.def))
      return build_fp_any_tables(c, any);
    release_fp_any(c);
  }
  return TE_OK;
}

void rebuild_footprint_tables(te_ctx* c) {
  c->fp_tables_ready = false;
  const int rc = rebuild_footprint_tables_impl(c);
  c->fp_tables_rc = rc;
  if (rc) {
    snprintf(c->fp_tables_err, sizeof(c->fp_tables_err), "%s", g_err);
    (void)hipGetLastError();
  } else {
    c->fp_tables_ready = true;
  }
}

int rebuild_tables(te_ctx* c) {
  c->tables_ready = false;
  c->fp_tables_ready = false;
  drop_graph(c);  // kernel arguments (disc tables, grids) are baked into the captured launches
  if (!c->have_params || !c->have_geo) return TE_OK;
  const te_params& p = c->params;
  const double res = c->geo.res;
  int rc;
  if ((rc = filter_disc(c, p.normals_radius, &c->cp.normals, &c->fa_host[0], "normals"))) return rc;
  if ((rc = filter_disc(c, p.rough_radius, &c->cp.rough, &c->fa_host[1], "roughness estimation"))) return rc;
  if ((rc = filter_disc(c, p.step_radius1, &c->cp.step1, &c->fa_host[2], "step first window"))) return rc;
  if ((rc = filter_disc(c, p.step_radius2, &c->cp.step2, &c->fa_host[3], "step second window"))) return rc;
  if ((rc = upload_any_discs(c))) return rc;
  if (c->cp.normals.any || c->cp.rough.any)
    c->cp.same_rough_disc = c->cp.normals.any && c->cp.rough.any && same_disc_table(c->fa_host[0], c->fa_host[1]) ? 1 : 0;
  else
    c->cp.same_rough_disc = same_disc(c->cp.normals, c->cp.rough) ? 1 : 0;
  c->cp.axis = p.normals_axis;
  c->cp.slope_crit = p.slope_critical;
  c->cp.step_crit = p.step_critical;
  c->cp.rough_crit = p.rough_critical;
  c->cp.step_ncrit = p.step_ncrit;
  c->cp.w_scale = p.w_scale;
  c->cp.w_slope = p.w_slope;
  c->cp.w_step = p.w_step;
  c->cp.w_rough = p.w_rough;
  // x/y moments of the normals disc clipped by the map border, for the sliding-disc kernel
  // (a tie radius: the table of the disc WITH the cells on its circle behind it, then the circle's offsets with both
  // parts non-zero -- te_normals3.hip, TIES march)
  // (a disc of te_filter_any.hip has no clip table)
  if (!c->cp.normals.any && (c->cp.normals.R >= 1 || c->cp.normals.n_ties != 0)) {
    const Disc& dn = c->cp.normals;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->cmem.clip_table.once(sizeof(int) * (2 * fast::kClipInts + kMaxTies)));
    int* const clip_table = c->cmem.clip_table.as<int>();
    // tie-free: the disc's table at R = dn.R, first; a tie radius: the full table at R = dn.reach, second, and no first one
    const bool ties = dn.n_ties != 0;
    const int R = ties ? dn.reach : dn.R;
    TieCircle tc;
    if (ties) build_tie_circle(dn, &tc);
    std::vector<int> tab((size_t)(2 * R + 1) * (2 * R + 1) * 6);
    build_clip_table(ties ? tc.full : dn, R, tab.data());
    HIP_TRY(hipMemcpyAsync(clip_table + (ties ? fast::kClipInts : 0), tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    if (ties && tc.n_gen) HIP_TRY(hipMemcpyAsync(clip_table + 2 * fast::kClipInts, tc.gen, tc.n_gen * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  c->L.clip_table = c->cmem.clip_table.as<int>();
  HIP_TRY(hipSetDevice(c->device));
  chain_route_template(c->geo, c->cp);  // (what plan_chain_route asks of the discs and the map: once, not per launch)

  c->tables_ready = true;
  rebuild_footprint_tables(c);
  return TE_OK;
}

void free_layers(te_ctx* c) {
  drop_graph(c);
  c->lmem = te_ctx::LayerMem();  // every buffer of the group, the spiral tables of the path checks (clipped to the map) included
  // ... and what pointed into them: the slab's parts (c->L with its tie_scratch, c->face_flags), the second polygon layer,
  // the tables of the route of any reach (their prefix sums are sized by the geometry; rebuilt with the tables)
  memset(&c->L, 0, sizeof(c->L));
  c->face_flags = nullptr;
  c->poly_rot = nullptr;
  clear_fp_any_ptrs(c);
  c->fill_mask_valid.clear();  // (lmem.median_mask is gone)
  guard_cache_generation().fetch_add(1, std::memory_order_acq_rel);  // (layer_has_guard_rows: verdicts about freed memory)
  c->layer_elems = 0;
  c->st.layers_freed();
}

float* layer_ptr(te_ctx* c, int layer) {
  switch (layer) {
    case TE_LAYER_ELEVATION: return c->L.elev;
    case TE_LAYER_SLOPE: return c->L.slope;
    case TE_LAYER_STEP: return c->L.step;
    case TE_LAYER_ROUGHNESS: return c->L.rough;
    case TE_LAYER_TRAVERSABILITY: return c->L.trav;
    case TE_LAYER_FOOTPRINT: return c->L.footprint;
    case TE_LAYER_NORMAL_X: return c->L.nx;
    case TE_LAYER_NORMAL_Y: return c->L.ny;
    case TE_LAYER_NORMAL_Z: return c->L.nz;
    case TE_LAYER_SLOPE_FOOTPRINT: return c->L.slope_fp;
    case TE_LAYER_STEP_FOOTPRINT: return c->L.step_fp;
    case TE_LAYER_ROUGHNESS_FOOTPRINT: return c->L.rough_fp;
    case TE_LAYER_TRAVERSABILITY_X: return c->lmem.poly.as<float>();
    case TE_LAYER_TRAVERSABILITY_ROT: return c->poly_rot;
    case TE_LAYER_ROBOT_SLOPE: return c->lmem.robot_slope.as<float>();
    default: return c->user.added(layer) ? c->lmem.user[layer - TE_LAYER_COUNT].as<float>() : nullptr;  // (a user layer, or no layer)
  }
}

layer_call::Facts facts_of(const te_ctx* c) {
  layer_call::Facts f;
  f.have_geo = c->have_geo;
  f.batch = c->geo.batch;
  f.rows = c->geo.rows;
  f.cols = c->geo.cols;
  for (int id = 0; id < TE_LAYER_COUNT + TE_MAX_USER_LAYERS; ++id)
    if (layer_ptr(const_cast<te_ctx*>(c), id)) f.has_memory |= bit(id);  // (layer_ptr only reads)
  f.layers_written = c->st.layers_written();
  f.have_robot_slope = c->st.have_robot_slope();
  f.have_elev = c->st.have_elev();
  f.user_added = c->user.mask();
  return f;
}

int refused(const char* who, const te_ctx* c, const layer_call::Verdict& v, const CallWhere& at) {
  switch (v.rule) {
    case layer_call::kAccepted: return TE_OK;
    case layer_call::kNoGeometry: return fail(v.code, "%s: geometry not set", who);
    case layer_call::kBadOutput: return fail(v.code, "%s: bad output layer %d", who, v.id);
    case layer_call::kBadMaps: return fail(v.code, "%s: maps [%d,%d) of batch %d", who, at.map0, at.map0 + at.nmaps, c->geo.batch);
    case layer_call::kTooManyMaps: return fail(v.code, "%s: %d maps in one call (at most %d)", who, at.nmaps, at.max_maps);
    case layer_call::kBadInput: return fail(v.code, "%s: bad input layer %d", who, v.id);
    case layer_call::kInputAbsent: return fail(v.code, "%s: the input layer %d does not exist yet", who, v.id);
    case layer_call::kOutputNoMemory: return fail(v.code, "%s: the output layer %d has no memory yet", who, v.id);
    case layer_call::kBadMap: return fail(v.code, "%s: map %d of batch %d", who, at.map0, c->geo.batch);
    case layer_call::kRegionInPlace:
      return fail(v.code, "%s: in_layer == out_layer (%d): a region call reads the neighbours of the rectangle as they were before "
                          "the filter, and in place their earlier input is gone; keep the unfiltered values in a layer of their own", who, v.id);
    case layer_call::kBadRect:
      return fail(v.code, "%s: rectangle (%d,%d)+(%d,%d) outside %dx%d", who, at.row0, at.col0, at.h, at.w, c->geo.rows, c->geo.cols);
    case layer_call::kOperandAbsent: return fail(v.code, "%s: the layer %s does not exist yet", who, layer_name_of(c, v.id));
  }
  return fail(TE_ERR_INVALID_ARG, "%s: refused", who);  // (never: every rule has its case)
}

int read_block_counts(te_ctx* c, const DevBuf& counts, uint64_t out[2]) {
  HIP_TRY(hipSetDevice(c->device));
  unsigned long long h[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(h, counts.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  out[0] = h[0];
  out[1] = h[1];
  return TE_OK;
}

int readable_layer(const char* who, te_ctx* c, int layer, float** out) {
  float* const p = layer_ptr(c, layer);
  if (c->user.added(layer) && (!p || !(c->st.layers_written() & bit(layer))))
    return fail(TE_ERR_NOT_READY, "%s: the layer %s does not exist yet (nothing has written it)", who, layer_name_of(c, layer));
  if (!p) return fail(TE_ERR_INVALID_ARG, "%s: bad layer %d", who, layer);
  *out = p;
  return TE_OK;
}

void snapshot_user_names(te_ctx* c, UserNames* out) {
  std::lock_guard<std::mutex> lk(c->mu);
  out->copy = c->user;
  out->n = out->copy.operands(out->v);
}

const char* layer_name_of(const te_ctx* c, int layer) {
  int n = 0;
  const expr::LayerName* names = expr::layer_names(&n);
  if (layer >= 0 && layer < n) return names[layer].name;
  return c->user.added(layer) ? c->user.name[layer - TE_LAYER_COUNT] : "(no layer)";
}

// the optional input layer robot_slope exists from its first upload on (every cell NaN = not valid until written), and so
// does every user layer
int ensure_input_layer(te_ctx* c, int layer) {
  c->st.layer_touched(layer);
  if (!layer_on_demand(c, layer)) return TE_OK;
  DevBuf& rs = layer == TE_LAYER_ROBOT_SLOPE ? c->lmem.robot_slope : c->lmem.user[layer - TE_LAYER_COUNT];
  if (rs.p) return TE_OK;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(rs.once(c->layer_elems * sizeof(float)));
  const hipError_t e = hipMemsetD32Async((hipDeviceptr_t)rs.p, 0x7fc00000, c->layer_elems, c->stream);
  if (e != hipSuccess) {
    rs.release();
    return fail(TE_ERR_HIP, "layer %s: %s", layer_name_of(c, layer), hipGetErrorString(e));
  }
  return TE_OK;
}

// The launch wrappers of the filters return hipErrorInvalidValue for a planned route without its instantiation
// (te_chain_route.h): an internal routing error, not a failure of the runtime
#define ROUTE_TRY(expr, what)                                                                              \
  do {                                                                                                     \
    if ((expr) == hipErrorInvalidValue) {                                                                  \
      (void)hipGetLastError();                                                                             \
      return fail(TE_ERR_UNSUPPORTED, "%s: the planned kernel route has no instantiation: internal routing error", what); \
    }                                                                                                      \
  } while (0)

int run_chain_locked(te_ctx* c, unsigned flags, const Region& r) {
  if (!c->have_params || !c->have_geo) return fail(TE_ERR_NOT_READY, "te_run_chain: set params and geometry first");
  if (!c->tables_ready) {
    int rc = rebuild_tables(c);
    if (rc) return rc;
  }
  if (!c->st.have_elev()) return fail(TE_ERR_NOT_READY, "te_run_chain: no elevation uploaded");
  if (int rc = refuse_rank_rule(c)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  // Two streams (step filter || normals kernel) pay from about 2^21 cells: below that the launch is a handful of
  // short kernels and the fork / join events cost more than the overlap gains -- one stream, the combine fused into the
  // normals kernel (MI355X, R = 5, chain: 256^2 0.045 -> 0.030 ms, 512^2 0.042 -> 0.032, 1024^2 0.052 -> 0.046, 2048^2 equal).
  static const bool force_two = lab_flag("TE_TWO_STREAMS");  // measurement aid
  const bool small = !force_two && (size_t)c->geo.rows * c->geo.cols * c->geo.batch < ((size_t)1 << 21);
  c->L.aux_stream = ((flags & TE_RUN_SEQUENTIAL) || small) ? nullptr : c->aux_stream;
  // whole-map run with the footprint pass right behind: the mask kernel writes the combined layer
  if (flags & TE_RUN_NORMALS_ONLY) flags &= ~(TE_RUN_FOOTPRINT | TE_RUN_FOOTPRINT_MEMO);
  // (only if the footprint pass can run at all: with a footprint this build cannot handle the combined layer would
  // never be written)
  if ((flags & TE_RUN_FOOTPRINT) && !c->fp_tables_ready)
    return fail(c->fp_tables_rc ? c->fp_tables_rc : TE_ERR_NOT_READY, "%s", c->fp_tables_err[0] ? c->fp_tables_err : "footprint tables not built");
  const bool whole = r.map < 0;
  if (c->st.chain_launching(whole, flags)) flags |= kDeferCombine;
  c->L.ev_fork = c->ev_fork;
  c->L.ev_join = c->ev_join;
  c->L.fb_walk = c->opt_fb_walk;
  c->L.fb_blocks_per_cu = c->opt_fb_blocks_per_cu;
  set_launch_hints(c);  // (run_whole_locked allocates their buffers before it captures)
  if (c->opt_rank_rule && !c->opt_normals_raster) flags |= TE_RUN_GENERIC_KERNELS;  // (the rule lives in the generic normals kernel only)
  const hipError_t e = launch_chain(c->geo, c->cp, c->L, r, flags, c->stream);
  ROUTE_TRY(e, "te_run_chain");
  HIP_TRY(e);
  c->st.chain_launched(whole, flags);
  return TE_OK;
}

// bound of the combined layer for a footprint pass that is about to run (te_ctx_state.h: trav_cap); < 0: none
static double trav_cap_now(const te_ctx* c, bool fresh) { return c->st.trav_cap(c->cp.w_scale, c->cp.w_slope, c->cp.w_step, c->cp.w_rough, fresh); }

// fresh: called right behind a whole-map chain in the same entry point (the combined layer is the chain's, cell for cell)
int run_footprint_locked(te_ctx* c, unsigned flags, bool fresh = false) {
  if (!c->st.chain_done() || !c->tables_ready)
    return fail(TE_ERR_NOT_READY, "te_run_footprint: run the filter chain first (it produces the layers the footprint reads)");
  if (!c->fp_tables_ready) return fail(c->fp_tables_rc ? c->fp_tables_rc : TE_ERR_NOT_READY, "%s", c->fp_tables_err);
  HIP_TRY(hipSetDevice(c->device));
  const double trav_cap = trav_cap_now(c, fresh);
  const bool memo = (flags & TE_RUN_FOOTPRINT_MEMO) != 0;
  if (int rc = ensure_fp_any(c, trav_cap)) return rc;
  HIP_TRY(launch_footprint(c->geo, c->fp, c->L, usable_face_flags(c), c->cmem.spiral.as<unsigned>(), c->cmem.fp_clip_table.as<int>(), memo,
                           c->st.combine_deferred() ? &c->cp : nullptr, trav_cap, c->stream));
  c->st.footprint_launched(memo);
  return TE_OK;
}

// Whole-map chain (+ footprint): the launch sequence is captured once per (flags, hole hints) into a hipGraph and replayed
// from 2^22 cells on (TE_OPT_GRAPH_REPLAY: always / never).  Measured on MI355X / ROCm 7.2, direct -> replayed, us per launch
// (tools/lab/graph_small_ab.py, round 6): bag map 17 -> 23, 256^2 25 -> 31, 1024^2 45 -> 52 (the replay costs 6 us on a
// launch that is a handful of short kernels on one stream), 2048^2 85 -> 79 and 121 -> 118 with the footprint pass, 4096^2
// 17 us saved (round 1).  Any capture problem switches the context back to direct launches for good.
int run_whole_locked(te_ctx* c, unsigned flags) {
  const Region r = {-1, 0, 0, c->geo.rows, c->geo.cols};
  static const bool no_graph = lab_flag("TE_NO_GRAPH");
  const bool large = c->opt_graph == 1 || (c->opt_graph == 0 && (size_t)c->geo.rows * c->geo.cols * c->geo.batch >= ((size_t)1 << 22));
  // (only the defined TE_RUN_* bits: the graph key below puts its own hints into the upper bits of the same word)
  flags &= TE_RUN_KEEP_NORMALS | TE_RUN_FOOTPRINT | TE_RUN_GENERIC_KERNELS | TE_RUN_FOOTPRINT_MEMO | TE_RUN_SEQUENTIAL | TE_RUN_NORMALS_ONLY;
  if (c->opt_rank_rule && !c->opt_normals_raster) flags |= TE_RUN_GENERIC_KERNELS;
  if (flags & TE_RUN_NORMALS_ONLY) flags &= ~(TE_RUN_FOOTPRINT | TE_RUN_FOOTPRINT_MEMO);
  if (!no_graph && large && !(flags & TE_RUN_NORMALS_ONLY) && c->graph_ok && c->have_params && c->have_geo && c->st.have_elev()) {
    if (!c->tables_ready) {
      int rc = rebuild_tables(c);
      if (rc) return rc;
    }
    if (int rc = refuse_rank_rule(c)) return rc;  // (before a capture: a failed one would end graph replay for good)
    HIP_TRY(hipSetDevice(c->device));
    int slot = -1;
    // (the captured launches bake in which k_normals3 variant runs, and whether the mask kernel is given the face flags: the
    // hints are part of the key; asking for them here allocates their buffers before the capture)
    const unsigned key = flags | launch_hints(c).key_bits(flags);
    for (int k = 0; k < te_ctx::kGraphs; ++k)
      if (c->graph_exec[k] && c->graph_flags[k] == key) slot = k;
    if (slot < 0) {
      slot = c->graph_next;
      c->graph_next = (c->graph_next + 1) % te_ctx::kGraphs;
      if (c->graph_exec[slot]) (void)hipGraphExecDestroy(c->graph_exec[slot]);
      c->graph_exec[slot] = nullptr;
      hipGraph_t graph = nullptr;
      int rc = TE_OK;
      hipError_t e = hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed);
      if (e == hipSuccess) {
        rc = run_chain_locked(c, flags, r);
        if (!rc && (flags & TE_RUN_FOOTPRINT)) rc = run_footprint_locked(c, flags, true);
        e = hipStreamEndCapture(c->stream, &graph);
      }
      if (e == hipSuccess && rc == TE_OK && graph) e = hipGraphInstantiate(&c->graph_exec[slot], graph, nullptr, nullptr, 0);
      if (graph) (void)hipGraphDestroy(graph);
      if (e != hipSuccess || rc != TE_OK || !c->graph_exec[slot]) {
        (void)hipGetLastError();
        drop_graph(c);
        c->graph_ok = false;
        slot = -1;
      } else {
        c->graph_flags[slot] = key;
      }
    }
    if (slot >= 0) {
      TraceRange tr("te_run_chain: graph replay (chain + footprint kernels)");
      HIP_TRY(hipGraphLaunch(c->graph_exec[slot], c->stream));
      c->st.graph_replayed(flags);
      return TE_OK;
    }
  }
  int rc = run_chain_locked(c, flags, r);
  if (!rc && (flags & TE_RUN_FOOTPRINT)) rc = run_footprint_locked(c, flags, true);
  return rc;
}

int sync_tiles(te_ctx* c) {  // the copy streams of the streaming-tile calls
  if (!c->tiles_pending) return TE_OK;
  if (c->in_stream) HIP_TRY(hipStreamSynchronize(c->in_stream));
  if (c->out_stream) HIP_TRY(hipStreamSynchronize(c->out_stream));
  c->tiles_pending = false;
  return TE_OK;
}

}  // namespace shim
}  // namespace te

extern "C" {

const char* te_last_error(void) { return g_err; }
const char* te_version(void) { return "travgpu 0.1 (gfx950)"; }

int te_params_default(te_params* p) {
  if (!p) return fail(TE_ERR_INVALID_ARG, "te_params_default: NULL");
  memset(p, 0, sizeof(*p));
  p->size = (uint32_t)sizeof(te_params);
  p->abi_version = TE_ABI_VERSION;
  // traversability_estimation/config/robot_filter_parameter.yaml:3-33
  p->normals_radius = 0.05;
  p->normals_axis = 2;
  p->slope_critical = 1.0;
  p->step_critical = 0.12;
  p->step_radius1 = 0.04;
  p->step_radius2 = 0.04;
  p->step_ncrit = 4;
  p->rough_critical = 0.05;
  p->rough_radius = 0.05;
  p->w_scale = 1.0f / 3.0f;
  p->w_slope = p->w_step = p->w_rough = 1.0f;
  // robot_footprint_parameter.yaml:4-8, robot.yaml:10, TraversabilityMap.cpp:117-126
  p->fp_radius = 0.30;
  p->fp_offset = 0.15;
  p->fp_default = 0.3;
  p->fp_max_gap = 0.3;
  p->fp_critical_step = 0.12;
  p->fp_check_roughness = 0;
  return TE_OK;
}

int te_params_validate(const te_params* p) {
  if (!p) return fail(TE_ERR_INVALID_ARG, "te_params: NULL");
  if (p->size != sizeof(te_params) || p->abi_version != TE_ABI_VERSION)
    return fail(TE_ERR_INVALID_ARG, "te_params: size/abi mismatch (got %u/%u, want %zu/%d)", p->size, p->abi_version,
                sizeof(te_params), TE_ABI_VERSION);
  // same messages as the reference's configure()s
  if (!(p->slope_critical <= M_PI_2 && p->slope_critical >= 0.0))  // SlopeFilter.cpp:41
    return fail(TE_ERR_BAD_PARAM, "Critical slope must be in the interval [0, PI/2]");
  if (!(p->step_critical >= 0.0))  // StepFilter.cpp:45
    return fail(TE_ERR_BAD_PARAM, "Critical step height must be greater than zero.");
  if (!(p->step_radius1 >= 0.0))  // :58
    return fail(TE_ERR_BAD_PARAM, "'first_window_radius' must be greater than zero.");
  if (!(p->step_radius2 >= 0.0))  // :71
    return fail(TE_ERR_BAD_PARAM, "'second_window_radius' must be greater than zero.");
  if (p->step_ncrit <= 0)  // :84
    return fail(TE_ERR_BAD_PARAM, "'critical_cell_number' must be greater than zero.");
  if (!(p->rough_critical >= 0.0))  // RoughnessFilter.cpp:43
    return fail(TE_ERR_BAD_PARAM, "Critical roughness must be greater than zero");
  if (!(p->rough_radius >= 0.0))  // :55
    return fail(TE_ERR_BAD_PARAM, "Roughness estimation radius must be greater than zero");
  if (!(p->normals_radius >= 0.0)) return fail(TE_ERR_BAD_PARAM, "normals radius must not be negative");
  if (p->normals_axis < 0 || p->normals_axis > 2)
    return fail(TE_ERR_BAD_PARAM, "normal_vector_positive_axis must be x, y or z");
  if (!(p->fp_radius >= 0.0) || !(p->fp_offset >= 0.0))
    return fail(TE_ERR_BAD_PARAM, "footprint radius/offset must not be negative");
  if (!(p->fp_max_gap >= 0.0)) return fail(TE_ERR_BAD_PARAM, "max_gap_width must not be negative");
  return TE_OK;
}

int te_device_count(int* count) {
  if (!count) return fail(TE_ERR_INVALID_ARG, "te_device_count: NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return fail(TE_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
  }
  *count = n;
  return TE_OK;
}

int te_create(int device, te_ctx** out) {
  if (!out) return fail(TE_ERR_INVALID_ARG, "te_create: NULL out");
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return fail(TE_ERR_NO_DEVICE, "te_create: no HIP device visible (libtravgpu has no CPU fallback)");
  if (device < 0 || device >= n) return fail(TE_ERR_INVALID_ARG, "te_create: device %d of %d", device, n);
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(TE_ERR_NO_DEVICE, "te_create: device %d is %s; this library is built for gfx950 only", device,
                prop.gcnArchName);
  te_ctx* c = new (std::nothrow) te_ctx();
  if (!c) return fail(TE_ERR_INVALID_ARG, "te_create: out of host memory");
  c->device = device;
  memset(&c->L, 0, sizeof(c->L));
  memset(&c->geo, 0, sizeof(c->geo));
  memset(&c->cp, 0, sizeof(c->cp));
  memset(&c->fp, 0, sizeof(c->fp));
  te_params_default(&c->params);
  c->have_params = true;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreate(&c->ev0);
  if (e == hipSuccess) e = hipEventCreate(&c->ev1);
  if (e == hipSuccess) {  // the (shorter) step-filter kernels go first when both streams have work
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    e = hipStreamCreateWithPriority(&c->aux_stream, hipStreamNonBlocking, hi);
  }
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming);
  if (e != hipSuccess) {
    delete c;
    return fail(TE_ERR_HIP, "te_create: %s", hipGetErrorString(e));
  }
  *out = c;
  return TE_OK;
}

int te_destroy(te_ctx* c) {
  if (!c) return TE_OK;
  {
    CtxLock lk(c);
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->prefetch_thread.joinable()) {
      {
        std::lock_guard<std::mutex> pl(c->pf_mu);
        c->pf_quit = true;
      }
      c->pf_cv.notify_all();
      c->prefetch_thread.join();
    }
    free_layers(c);
    c->stager.release();
    c->prefetcher.release();
    if (c->prefetch_order) (void)hipStreamDestroy(c->prefetch_order);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->aux_stream) (void)hipStreamSynchronize(c->aux_stream);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->aux_stream) (void)hipStreamDestroy(c->aux_stream);
    for (hipStream_t st : {c->in_stream, c->out_stream})
      if (st) {
        (void)hipStreamSynchronize(st);
        (void)hipStreamDestroy(st);
      }
    c->cmem = te_ctx::CtxMem();  // (every stream has drained; the device is still current for `delete c`, which finds them empty)
    for (te_ctx::TileSlot* sl : {&c->in_slot[0], &c->in_slot[1], &c->out_slot[0], &c->out_slot[1]}) {
      if (sl->ready) (void)hipEventDestroy(sl->ready);
      if (sl->freed) (void)hipEventDestroy(sl->freed);
    }
    if (c->stream) (void)hipStreamDestroy(c->stream);
  }
  delete c;
  return TE_OK;
}

int te_set_params(te_ctx* c, const te_params* p) {
  if (!c) return fail(TE_ERR_INVALID_ARG, "te_set_params: NULL ctx");
  int rc = te_params_validate(p);
  if (rc) return rc;
  CtxLock lk(c, /*beside_prefetch*/ true);
  te_params old = c->params;
  c->params = *p;
  c->have_params = true;
  rc = rebuild_tables(c);
  if (rc) {
    c->params = old;
    (void)rebuild_tables(c);
    return rc;
  }
  // the filter layers stay valid when only the footprint part (fp_*, the tail of the struct) changed:
  // traversabilityFootprint(radius, offset) is called with a new radius on an unchanged map
  // ... and the untraversable mask with them, unless one of the three parameters it reads changed; the face flags were built
  // for the critical step held at upload (te_face_flags.h): unknown until the next whole upload
  const bool crit_same = old.fp_critical_step == p->fp_critical_step;
  c->st.params_changed(memcmp(&old, p, offsetof(te_params, fp_radius)) != 0,
                       !(old.fp_max_gap == p->fp_max_gap && crit_same && old.fp_check_roughness == p->fp_check_roughness), !crit_same);
  return TE_OK;
}

int te_set_option(te_ctx* c, int option, int value) {
  if (!c) return fail(TE_ERR_INVALID_ARG, "te_set_option: NULL ctx");
  CtxLock lk(c);
  switch (option) {
    case TE_OPT_FP_BLOCKED_WALK:
      if (value < 0 || value > 2) return fail(TE_ERR_INVALID_ARG, "te_set_option: TE_OPT_FP_BLOCKED_WALK takes 0 (by list length), 1 (per wavefront), 2 (per lane)");
      c->opt_fb_walk = value;
      break;
    case TE_OPT_FP_BLOCKED_BLOCKS_PER_CU:
      if (value < 0 || value > 32) return fail(TE_ERR_INVALID_ARG, "te_set_option: TE_OPT_FP_BLOCKED_BLOCKS_PER_CU takes 0 (default) .. 32");
      c->opt_fb_blocks_per_cu = value;
      break;
    case TE_OPT_POLYGON_PER_CELL:
      c->opt_polygon_per_cell = value != 0;
      break;
    case TE_OPT_GRAPH_REPLAY:
      if (value < 0 || value > 2) return fail(TE_ERR_INVALID_ARG, "te_set_option: TE_OPT_GRAPH_REPLAY takes 0 (by size), 1 (always), 2 (never)");
      c->opt_graph = value;
      break;
    case TE_OPT_BCAST_RCCL:
      c->opt_bcast_rccl = value != 0;
      return TE_OK;  // (no launch depends on it)
    case TE_OPT_FP_ANY_REACH:
      if (value < 0 || value > 1) return fail(TE_ERR_INVALID_ARG, "te_set_option: TE_OPT_FP_ANY_REACH takes 0 (by reach) or 1 (every reach)");
      if (c->opt_fp_any != value) {
        c->opt_fp_any = value;
        c->st.footprint_option_changed();
        if (c->tables_ready) rebuild_footprint_tables(c);
      }
      break;
    case TE_OPT_FILTER_ANY_RADIUS:
      if (value < 0 || value > 2)
        return fail(TE_ERR_INVALID_ARG, "te_set_option: TE_OPT_FILTER_ANY_RADIUS takes 0 (up to 32 cells), 1 (any radius), 2 (the route of any radius for every disc)");
      if (c->opt_filter_any != value) {
        const int old = c->opt_filter_any;
        c->opt_filter_any = value;
        if (c->have_params && c->have_geo) {  // the discs of the parameters held; a failure leaves the option and the tables as they were
          const int rc = rebuild_tables(c);
          if (rc) {
            c->opt_filter_any = old;
            (void)rebuild_tables(c);
            return rc;
          }
        }
        c->st.filter_option_changed();
      }
      break;
    case TE_OPT_FACE_FLAGS:
      if (value < 0 || value > 1) return fail(TE_ERR_INVALID_ARG, "te_set_option: TE_OPT_FACE_FLAGS takes 0 (never passed to the mask kernel) or 1 (passed when known)");
      c->opt_face_flags = value;  // (identical layers either way: nothing computed so far is invalidated)
      break;
    case TE_OPT_MEDIAN_ROUTE:
      if (value < 0 || value > 2) return fail(TE_ERR_INVALID_ARG, "te_set_option: TE_OPT_MEDIAN_ROUTE takes 0 (by plan), 1 (the tile kernel wherever its window fits), 2 (the general kernel)");
      c->opt_median_route = value;
      return TE_OK;  // (read by te_run_median_fill alone, which is never captured; identical layers either way)
    case TE_OPT_RADIUS_ROUTE:
      if (value < 0 || value > 2) return fail(TE_ERR_INVALID_ARG, "te_set_option: TE_OPT_RADIUS_ROUTE takes 0 (by plan), 1 (the sliding kernel wherever it can run), 2 (the in-order gather)");
      c->opt_radius_route = value;
      return TE_OK;  // (read by te_run_radius_filter alone, which is never captured; identical layers either way)
    case TE_OPT_WINDOW_EXPR_ROUTE:
      if (value < 0 || value > 2) return fail(TE_ERR_INVALID_ARG, "te_set_option: TE_OPT_WINDOW_EXPR_ROUTE takes 0 (by plan), 1 (the separable route wherever allowed), 2 (the direct walk)");
      c->opt_window_expr_route = value;
      return TE_OK;  // (read by te_run_window_expression alone, which is never captured; identical layers either way)
    case TE_OPT_DISTANCE_ROUTE:
      if (value < 0 || value > 2) return fail(TE_ERR_INVALID_ARG, "te_set_option: TE_OPT_DISTANCE_ROUTE takes 0 (by plan), 1 (the tiled route wherever it fits), 2 (the route of any reach)");
      c->opt_distance_route = value;
      return TE_OK;  // (read by te_run_distance alone, which is never captured; identical layers either way)
    case TE_OPT_NORMALS_RANK_RULE:
      c->opt_rank_rule = value != 0;
      c->st.filter_option_changed();
      break;
    case TE_OPT_NORMALS_ALGORITHM:
      if (value < 0 || value > 1) return fail(TE_ERR_INVALID_ARG, "te_set_option: TE_OPT_NORMALS_ALGORITHM takes 0 (area) or 1 (raster)");
      if (c->opt_normals_raster == value) return TE_OK;  // (the plugins set it before every update: nothing to drop)
      c->opt_normals_raster = value;
      c->st.normals_algorithm_set();
      break;  // (the captured launches are dropped below)
    default:
      return fail(TE_ERR_INVALID_ARG, "te_set_option: unknown option %d", option);
  }
  drop_graph(c);  // (captured launches bake the choice in)
  return TE_OK;
}

int te_download_face_flags(te_ctx* c, unsigned char* out, size_t bytes) {
  if (!c || !out) return fail(TE_ERR_INVALID_ARG, "te_download_face_flags: NULL");
  CtxLock lk(c);
  const uint8_t* f = c->have_geo && c->st.have_elev() ? usable_face_flags(c) : nullptr;
  if (!f) return fail(TE_ERR_NOT_READY, "te_download_face_flags: the face flags of the elevation layer are unknown or switched off");
  const size_t n = face_flag_bytes(c->geo.rows, c->geo.cols, c->geo.batch);
  if (bytes != n) return fail(TE_ERR_INVALID_ARG, "te_download_face_flags: %zu bytes given, the flags are %zu", bytes, n);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(out, f, n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return TE_OK;
}

int te_get_params(te_ctx* c, te_params* p) {
  if (!c || !p) return fail(TE_ERR_INVALID_ARG, "te_get_params: NULL");
  CtxLock lk(c, /*beside_prefetch*/ true);
  *p = c->params;
  return TE_OK;
}

int te_set_geometry(te_ctx* c, int rows, int cols, int batch, double res, double pos_x, double pos_y) {
  if (!c) return fail(TE_ERR_INVALID_ARG, "te_set_geometry: NULL ctx");
  if (rows <= 0 || cols <= 0 || batch <= 0 || !(res > 0.0) || !isfinite(res) || !isfinite(pos_x) || !isfinite(pos_y))
    return fail(TE_ERR_INVALID_ARG, "te_set_geometry: rows=%d cols=%d batch=%d res=%g", rows, cols, batch, res);
  CtxLock lk(c);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const size_t elems = (size_t)rows * cols * batch;
  // a new shape always gets a fresh slab: the fix-up flag array is sized from (rows, cols, batch), not from the cell
  // count (a transposed map of equal size needs a different number of 64x16 tiles), and layers computed for another
  // shape must not be served as if they belonged to this one
  if (elems != c->layer_elems || rows != c->geo.rows || cols != c->geo.cols || batch != c->geo.batch) {
    free_layers(c);
    // one slab (te_slab.h: the plan of its parts, with kSlabGuardRows rows of slack before the first and behind the last)
    Geo gtmp;
    gtmp.rows = rows;
    gtmp.cols = cols;
    gtmp.batch = batch;
    const SlabPlan sp = plan_slab(rows, cols, batch, (size_t)fast::normals_fast_max_blocks(gtmp), fast::fp_list_slack(rows, cols, batch, device_cus()),
                                  untrav_flag_bytes(rows, cols, batch), face_flag_bytes(rows, cols, batch));
    const hipError_t e = c->lmem.slab.once(sp.total);
    if (e != hipSuccess) return fail(TE_ERR_HIP, "te_set_geometry: hipMalloc(%zu bytes): %s", sp.total, hipGetErrorString(e));
    char* const slab = c->lmem.slab.as<char>();
    float** ptrs[kSlabFloatLayers] = {&c->L.elev, &c->L.slope, &c->L.step,     &c->L.rough,   &c->L.trav,     &c->L.footprint, &c->L.nx,
                                      &c->L.ny,   &c->L.nz,    &c->L.slope_fp, &c->L.step_fp, &c->L.rough_fp, &c->L.step_height};
    for (int k = 0; k < kSlabFloatLayers; ++k) *ptrs[k] = (float*)(slab + sp.layer_off(k));
    // (the list of cells with an untraversable cell in their disc holds 32-bit entries: absent beyond them)
    const bool have_list = sp.list_cap < ((size_t)1 << 32);
    c->L.untrav = (uint8_t*)(slab + sp.mask.off);
    c->L.block_flags = (int*)(slab + sp.fix_flags.off);
    c->L.fp_blocked = have_list ? (unsigned*)(slab + sp.list.off) : nullptr;
    c->L.fp_blocked_count = (unsigned*)(slab + sp.list_count.off);
    c->L.fp_blocked_cap = sp.list_cap;
    c->L.untrav_flags = (uint8_t*)(slab + sp.untrav_flags.off);
    c->L.fp_scratch = have_list ? (unsigned*)(slab + sp.sum_scratch.off) : nullptr;  // (the sum kernel's, see Layers::fp_scratch)
    c->face_flags = (uint8_t*)(slab + sp.face_flags.off);  // (te_face_flags.h, written by the upload's pass)
    c->layer_elems = elems;
    // outputs read as NaN until computed, like GridMap::add(): the front guard, the layers, the mask and the fix-up flags ...
    HIP_TRY(hipMemsetAsync(slab, 0xFF, sp.list.off, c->stream));
    HIP_TRY(hipMemsetAsync(slab + sp.back_guard.off, 0xFF, sp.back_guard.bytes, c->stream));
    // (the flag grids: 1 = "holds an untraversable cell" / "a vertical face", unknown until their kernels have written them)
    HIP_TRY(hipMemsetAsync(c->face_flags, 0x01, sp.face_flags.bytes, c->stream));
    HIP_TRY(hipMemsetAsync(c->L.untrav_flags, 0x01, sp.untrav_flags.bytes, c->stream));
    // the mask layer holds 0 / 1 only (k_fp_slide5 packs the byte as it is): "untraversable" until the mask kernel has
    // looked at the cell, as a byte of 0xFF would also say -- but 1 stays inside the packed word's flag bit
    HIP_TRY(hipMemsetAsync(c->L.untrav, 0x01, sp.mask.bytes, c->stream));
    HIP_TRY(hipMemsetAsync(c->L.fp_blocked_count, 0, sp.list_count.bytes, c->stream));
    // the fix-up flags are zero between launches: k_normals_fixup clears every flag it consumes
    HIP_TRY(hipMemsetAsync(c->L.block_flags, 0, sp.fix_flags.bytes, c->stream));
  }
  c->geo.rows = rows;
  c->geo.cols = cols;
  c->geo.batch = batch;
  c->geo.res = res;
  c->geo.len_x = (double)rows * res;  // GridMap::setGeometry: length = size * resolution
  c->geo.len_y = (double)cols * res;
  c->geo.pos_x = pos_x;
  c->geo.pos_y = pos_y;
  c->geo.ax = pos_x + (0.5 * c->geo.len_x - 0.5 * res);
  c->geo.ay = pos_y + (0.5 * c->geo.len_y - 0.5 * res);
  c->have_geo = true;
  c->st.geometry_set();
  c->fill_mask_valid.clear();  // (te_download_fill_mask: the mask of a fill under another geometry is not this map's)
  return rebuild_tables(c);
}

int te_run_filter(te_ctx* c, int filter, unsigned flags) {
  if (!c) return fail(TE_ERR_INVALID_ARG, "te_run_filter: NULL ctx");
  static const char* const kFilterRange[] = {"te_run_filter", "te_run_filter: slope", "te_run_filter: step", "te_run_filter: roughness",
                                             "te_run_filter: combine", "te_run_filter: normals"};
  TraceRange tr(kFilterRange[(filter >= 0 && filter < 6) ? filter : 0]);
  CtxLock lk(c, /*beside_prefetch*/ true, filter_layers(filter));
  if (!c->have_geo || !c->have_params) return fail(TE_ERR_NOT_READY, "te_run_filter: set params and geometry first");
  if (!c->tables_ready) {
    int rc = rebuild_tables(c);
    if (rc) return rc;
  }
  if (filter < TE_FILTER_SLOPE || filter > TE_FILTER_NORMALS) return fail(TE_ERR_INVALID_ARG, "te_run_filter: bad filter %d", filter);
  if ((filter == TE_FILTER_STEP || filter == TE_FILTER_ROUGHNESS || filter == TE_FILTER_NORMALS) && !c->st.have_elev())
    return fail(TE_ERR_NOT_READY, "te_run_filter: no elevation uploaded");
  if (filter == TE_FILTER_NORMALS)
    if (int rc = refuse_rank_rule(c)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  set_launch_hints(c);  // (as in the chain: never stale ones)
  if (c->opt_rank_rule && !c->opt_normals_raster) flags |= TE_RUN_GENERIC_KERNELS;
  const hipError_t e = launch_filter(c->geo, c->cp, c->L, filter, flags, c->stream);
  ROUTE_TRY(e, "te_run_filter");
  HIP_TRY(e);
  c->st.filter_ran(filter);
  return TE_OK;
}

int te_run_chain(te_ctx* c, unsigned flags) {
  if (!c) return fail(TE_ERR_INVALID_ARG, "te_run_chain: NULL ctx");
  TraceRange tr("te_run_chain");
  CtxLock lk(c);
  if (!c->have_geo) return fail(TE_ERR_NOT_READY, "te_run_chain: geometry not set");
  return run_whole_locked(c, flags);
}

// te_run_chain_region and te_run_chain_region_expression under the caller's lock.  prog (nullptr: the weighted sum the chain
// writes) is evaluated on the rectangle the chain recombines -- the region grown by the chain's reach -- behind the chain and
// before the footprint half.
static int chain_region_locked(const char* who, te_ctx* c, unsigned flags, const expr::Program* prog, int map, int row0, int col0, int h, int w) {
  if (!c->have_geo) return fail(TE_ERR_NOT_READY, "%s: geometry not set", who);
  if (map < 0 || map >= c->geo.batch || row0 < 0 || col0 < 0 || h <= 0 || w <= 0 || row0 + h > c->geo.rows ||
      col0 + w > c->geo.cols)
    return fail(TE_ERR_INVALID_ARG, "%s: rectangle outside the map", who);
  if (c->opt_normals_raster)
    return fail(TE_ERR_UNSUPPORTED, "%s: not built under TE_OPT_NORMALS_ALGORITHM = 1 (raster): the roughness route on given "
                                    "normals is whole-map only; run te_run_chain", who);
  if (!c->st.chain_done()) return fail(TE_ERR_NOT_READY, "%s: run the full chain once first", who);
  const Region r = {map, row0, col0, row0 + h, col0 + w};
  const bool want_fp = (flags & (TE_RUN_FOOTPRINT | TE_RUN_FOOTPRINT_MEMO)) != 0;
  const bool fp_was_done = c->st.footprint_done(), mask_was_done = c->st.mask_done();
  if (want_fp && !fp_was_done)
    return fail(TE_ERR_NOT_READY, "%s: the footprint flag refreshes a complete traversability_footprint layer; run the "
                                  "whole-map footprint pass once first (te_run_chain with TE_RUN_FOOTPRINT, or te_run_footprint)", who);
  expr::Args ea;
  if (prog)  // (a missing layer is refused before the chain is launched)
    if (const int rc = region_expression_args(who, c, *prog, &ea)) return rc;
  int rc = run_chain_locked(c, flags & ~(TE_RUN_FOOTPRINT | TE_RUN_FOOTPRINT_MEMO), r);
  if (rc) return rc;
  const int reach = chain_max_reach(c->cp);
  auto grown = [&](int k) {
    Region o = r;
    o.i0 = r.i0 - k < 0 ? 0 : r.i0 - k;
    o.j0 = r.j0 - k < 0 ? 0 : r.j0 - k;
    o.i1 = r.i1 + k > c->geo.rows ? c->geo.rows : r.i1 + k;
    o.j1 = r.j1 + k > c->geo.cols ? c->geo.cols : r.j1 + k;
    return o;
  };
  if (prog && !(flags & TE_RUN_NORMALS_ONLY)) {
    // the chain's weighted sum on r_combine (te_chain_route.h: plan_rects) is overwritten by the expression, cell for cell
    const Region rc_ = grown(reach);
    if (const int rc2 = region_expression_launch(who, c, *prog, ea, map, rc_.i0, rc_.j0, rc_.i1 - rc_.i0, rc_.j1 - rc_.j0)) return rc2;
  }
  if (!want_fp) return TE_OK;
  // The scores changed within the chain's reach of the rectangle (launch_chain re-filters and re-combines exactly that);
  // the footprint pass follows on the cells that can see them.
  // (checkForStep also follows a ray of up to max_gap_width and a Bresenham line along it through the ELEVATION, which
  // changed in the rectangle itself: the mask of a cell depends on elevations up to 2.5 + 1 + max_gap/res cells away; the
  // mask is recomputed within 3 cells of `changed`)
  const int gap_cells = (int)ceil(c->params.fp_max_gap / c->geo.res) + 5;
  const Region changed = grown(reach > gap_cells - 3 ? reach : gap_cells - 3);
  // (behind an expression the layer counts as written from outside: no bound, the route of any reach)
  const double trav_cap = trav_cap_now(c, /*fresh*/ false);
  if (int rc2 = ensure_fp_any(c, trav_cap)) return rc2;
  HIP_TRY(launch_footprint(c->geo, c->fp, c->L, usable_face_flags(c), c->cmem.spiral.as<unsigned>(), c->cmem.fp_clip_table.as<int>(), (flags & TE_RUN_FOOTPRINT_MEMO) != 0, nullptr, trav_cap,
                           c->stream, &changed));
  c->st.region_footprint_refreshed(mask_was_done);
  return TE_OK;
}

int te_run_chain_region(te_ctx* c, unsigned flags, int map, int row0, int col0, int h, int w) {
  if (!c) return fail(TE_ERR_INVALID_ARG, "te_run_chain_region: NULL ctx");
  TraceRange tr("te_run_chain_region");
  CtxLock lk(c);
  return chain_region_locked("te_run_chain_region", c, flags, nullptr, map, row0, col0, h, w);
}

int te_run_chain_region_expression(te_ctx* c, unsigned flags, const char* text, int map, int row0, int col0, int h, int w) {
  if (!text) return te_run_chain_region(c, flags, map, row0, col0, h, w);
  const char* const who = "te_run_chain_region_expression";
  if (!c) return fail(TE_ERR_INVALID_ARG, "%s: NULL ctx", who);
  expr::Program prog;
  if (const int rc = region_expression_program(who, text, &prog)) return rc;
  TraceRange tr(who);
  CtxLock lk(c);
  return chain_region_locked(who, c, flags, &prog, map, row0, col0, h, w);
}

int te_run_footprint(te_ctx* c) {
  if (!c) return fail(TE_ERR_INVALID_ARG, "te_run_footprint: NULL ctx");
  TraceRange tr("te_run_footprint");
  CtxLock lk(c);
  return run_footprint_locked(c, TE_RUN_FOOTPRINT_MEMO);
}

int te_sync(te_ctx* c) {
  if (!c) return fail(TE_ERR_INVALID_ARG, "te_sync: NULL ctx");
  CtxLock lk(c);
  HIP_TRY(hipSetDevice(c->device));
  // A blocking hipStreamSynchronize parks the thread and is woken by an interrupt; for the launches of this library
  // (a few hundred microseconds) that wake-up is a visible part of the latency, so the stream is polled first
  // (TE_SYNC_SPIN_US microseconds, default 2000; 0: block at once).
  static const long spin_us = lab_int("TE_SYNC_SPIN_US", 2000);
  if (spin_us > 0) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      const hipError_t e = hipStreamQuery(c->stream);
      if (e == hipSuccess) return sync_tiles(c);
      if (e != hipErrorNotReady) return fail(TE_ERR_HIP, "te_sync: %s", hipGetErrorString(e));
      if (std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > spin_us) break;
    }
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  return sync_tiles(c);
}

int te_time_chain(te_ctx* c, unsigned flags, int warmup, int iters, float* ms_per_iter) {
  if (!c || !ms_per_iter || iters <= 0 || warmup < 0) return fail(TE_ERR_INVALID_ARG, "te_time_chain: bad argument");
  CtxLock lk(c);
  if (!c->have_geo) return fail(TE_ERR_NOT_READY, "te_time_chain: geometry not set");
  for (int k = 0; k < warmup; ++k) {
    int rc = run_whole_locked(c, flags);
    if (rc) return rc;
  }
  HIP_TRY(hipEventRecord(c->ev0, c->stream));
  for (int k = 0; k < iters; ++k) {
    int rc = run_whole_locked(c, flags);
    if (rc) return rc;
  }
  HIP_TRY(hipEventRecord(c->ev1, c->stream));
  HIP_TRY(hipEventSynchronize(c->ev1));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  *ms_per_iter = ms / (float)iters;
  return TE_OK;
}

int te_time_chain_samples(te_ctx* c, unsigned flags, int warmup, int iters, float* ms) {
  if (!c || !ms || iters <= 0 || warmup < 0) return fail(TE_ERR_INVALID_ARG, "te_time_chain_samples: bad argument");
  CtxLock lk(c);
  if (!c->have_geo) return fail(TE_ERR_NOT_READY, "te_time_chain_samples: geometry not set");
  for (int k = 0; k < warmup; ++k) {
    int rc = run_whole_locked(c, flags);
    if (rc) return rc;
  }
  for (int k = 0; k < iters; ++k) {
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    int rc = run_whole_locked(c, flags);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev1));
    HIP_TRY(hipEventElapsedTime(&ms[k], c->ev0, c->ev1));
  }
  return TE_OK;
}

}  // extern "C"
