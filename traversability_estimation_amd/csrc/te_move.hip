// te_move.hip -- te_move_map: GridMap::move for the resident layers.  The shift, the rectangles and the launch geometry come
// from te_move_plan.h; the state change is te::CtxState::map_moved.  Semantics: include/travgpu.h.
//
// One layer of one map at a time is shifted OUT OF PLACE into the context's move scratch and copied back: the kernel reads
// the layer and writes the scratch only, so no workgroup reads a cell another one of the same launch may write, whatever the
// shift and the block order.  Every cell of the scratch is written -- the shifted value, or the fill where the source lies
// outside the old window -- and the copy back is one device-to-device transfer on the same stream.
#include "te_ctx.h"
#include "te_move_plan.h"
#include "te_slab.h"

using namespace te;
using namespace te::shim;

namespace te {
namespace move {
namespace {

// four cells at any cell boundary (the load) and at a boundary of four cells' bytes (the store)
template <class T>
struct Vec;
template <>
struct Vec<float> {
  typedef float loose __attribute__((ext_vector_type(4), aligned(4)));
  typedef float tight __attribute__((ext_vector_type(4), aligned(16)));
};
template <>
struct Vec<uint8_t> {
  typedef uint8_t loose __attribute__((ext_vector_type(4), aligned(1)));
  typedef uint8_t tight __attribute__((ext_vector_type(4), aligned(4)));
};

// dst (i, j) = src (i - sr, j - sc) where that is a cell of the rows x cols map -- rows [i_lo, i_hi), columns [j_lo, j_hi) of
// dst -- and `fill` elsewhere.  Columns are `rows` cells apart, so the alignment of a column changes from one to the next when
// rows is no multiple of four.  A column is cut for its DESTINATION as k_submap_pack cuts it: `head` cells up to the first
// boundary of four, then groups of four -- one load at whatever alignment the row shift leaves the source, one aligned store
// -- then up to three cells behind the last group.  Slot g of a column is group g; the two slots behind the largest possible
// group count take the head and the tail cell by cell.  A group that crosses i_lo or i_hi is assembled cell by cell and still
// stored whole.  The values move as bits.
// (The float instance compiles to global_load_dwordx4 / global_store_dwordx4.  The byte instance -- the two masks, a quarter
// of a float layer's bytes each -- keeps its aligned 4-byte store, but gfx950 has no unaligned dword load for a byte
// pointer and the compiler splits the load into four global_load_ubyte.)
template <class T>
__global__ __launch_bounds__(kLanes* kCols) void k_move_shift(const T* __restrict__ src, T* __restrict__ dst, int rows, int cols, int sr, int sc,
                                                              int i_lo, int i_hi, int j_lo, int j_hi, T fill) {
  typedef typename Vec<T>::loose VL;
  typedef typename Vec<T>::tight VT;
  constexpr unsigned kAlign = 4 * sizeof(T);
  const long long slots = (long long)(rows >> 2) + 2;
  for (long long j = (long long)blockIdx.y * kCols + threadIdx.y; j < cols; j += (long long)gridDim.y * kCols) {
    T* const d = dst + (size_t)j * (size_t)rows;
    const bool col_in = j >= j_lo && j < j_hi;
    // s[i] is the source of d[i]; only read for i in [i_lo, i_hi) of a column in [j_lo, j_hi): a cell of the source map
    const T* const s = src + ((long long)(col_in ? j - sc : 0) * (long long)rows - (long long)sr);
    auto cell = [&](int i) { return (col_in && i >= i_lo && i < i_hi) ? s[i] : fill; };
    int head = (int)(((kAlign - (unsigned)((uintptr_t)d & (kAlign - 1))) & (kAlign - 1)) / sizeof(T));
    if (head > rows) head = rows;
    const int ngroups = (rows - head) >> 2;
    for (long long g = (long long)blockIdx.x * kLanes + threadIdx.x; g < slots; g += (long long)gridDim.x * kLanes) {
      if (g < ngroups) {
        const int k = head + 4 * (int)g;
        if (col_in && k >= i_lo && k + 4 <= i_hi) {
          *(VT*)(d + k) = *(const VL*)(s + k);
        } else {
          VT v;
          v.x = cell(k), v.y = cell(k + 1), v.z = cell(k + 2), v.w = cell(k + 3);
          *(VT*)(d + k) = v;
        }
      } else if (g == slots - 2) {
        for (int k = 0; k < head; ++k) d[k] = cell(k);
      } else if (g == slots - 1) {
        for (int k = head + 4 * ngroups; k < rows; ++k) d[k] = cell(k);
      }
    }
  }
}

template <class T>
hipError_t shift_unit(const Plan& p, int rows, int cols, T* unit, T* scratch, T fill, hipStream_t stream) {
  hipLaunchKernelGGL(k_move_shift<T>, dim3(p.grid_x, p.grid_y), dim3(kLanes, kCols), 0, stream, (const T*)unit, scratch, rows, cols,
                     (int)p.info.shift_rows, (int)p.info.shift_cols, p.i_lo, p.i_hi, p.j_lo, p.j_hi, fill);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return hipMemcpyAsync(unit, scratch, (size_t)rows * (size_t)cols * sizeof(T), hipMemcpyDeviceToDevice, stream);
}

}  // namespace
}  // namespace move
}  // namespace te

extern "C" {

int te_move_geometry(int rows, int cols, double resolution, double pos_x, double pos_y, double new_x, double new_y, const te_params* params,
                     te_move_info* out) {
  if (!out) return fail(TE_ERR_INVALID_ARG, "te_move_geometry: NULL");
  move::Plan p;
  const char* why = "";
  if (const int rc = move::plan(rows, cols, resolution, pos_x, pos_y, new_x, new_y, params, false, &p, &why))
    return fail(rc, "te_move_geometry: %s", why);
  *out = p.info;
  return TE_OK;
}

int te_move_map(te_ctx* c, double new_x, double new_y, te_move_info* info) {
  if (!c) return fail(TE_ERR_INVALID_ARG, "te_move_map: NULL ctx");
  TraceRange tr("te_move_map");
  CtxLock lk(c);  // (joins a prefetch in flight: every layer is written)
  if (!c->have_geo) return fail(TE_ERR_NOT_READY, "te_move_map: geometry not set");
  const int rows = c->geo.rows, cols = c->geo.cols, batch = c->geo.batch;
  move::Plan p;
  const char* why = "";
  if (const int rc = move::plan(rows, cols, c->geo.res, c->geo.pos_x, c->geo.pos_y, new_x, new_y, c->have_params ? &c->params : nullptr,
                                c->opt_normals_raster != 0, &p, &why))
    return fail(rc, "te_move_map: %s", why);
  if (p.info.n_rects == 0) {  // a zero shift: nothing changes, not even the position
    if (info) *info = p.info;
    return TE_OK;
  }
  // every refusal comes before the first write
  if (c->layer_elems >= ((size_t)1 << 31))
    return fail(TE_ERR_UNSUPPORTED, "te_move_map: layers of %zu cells; maps of 2^31 cells and more are not moved", c->layer_elems);
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = (size_t)rows * (size_t)cols;
  if (p.scratch_bytes) {
    if (p.scratch_bytes != move_scratch_bytes(rows, cols)) return fail(TE_ERR_UNSUPPORTED, "te_move_map: scratch size: internal planning error");
    if (const int rc = reserve_scratch("te_move_map", c->lmem.move_scratch, p.scratch_bytes, c->stream, "the scratch of one layer of one map")) return rc;
  }
  if (info) *info = p.info;  // (behind the last refusal: a refused move hands out no rectangles)
  // the 15 public layers, the user layers and the step filter's height layer, wherever they have memory; the two byte masks
  float* layers[TE_LAYER_COUNT + TE_MAX_USER_LAYERS + 1];
  int n_layers = 0;
  for (int k = 0; k < TE_LAYER_COUNT + TE_MAX_USER_LAYERS; ++k)
    if (float* l = layer_ptr(c, k)) layers[n_layers++] = l;
  if (c->L.step_height) layers[n_layers++] = c->L.step_height;
  uint8_t* const masks[2] = {c->L.untrav, c->lmem.median_mask.as<uint8_t>()};
  const uint8_t mask_fill[2] = {1, 0};  // "untraversable until the mask kernel has looked at the cell" / shouldFill = 0
  if (p.info.all_exposed) {
    for (int k = 0; k < n_layers; ++k) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)layers[k], 0x7fc00000, c->layer_elems, c->stream));
    for (int k = 0; k < 2; ++k)
      if (masks[k]) HIP_TRY(hipMemsetAsync(masks[k], mask_fill[k], c->layer_elems, c->stream));
  } else {
    float* const scratch = c->lmem.move_scratch.as<float>();
    for (int k = 0; k < n_layers; ++k)
      for (int b = 0; b < batch; ++b) HIP_TRY(move::shift_unit<float>(p, rows, cols, layers[k] + n * (size_t)b, scratch, __builtin_nanf(""), c->stream));
    for (int k = 0; k < 2; ++k)
      for (int b = 0; masks[k] && b < batch; ++b)
        HIP_TRY(move::shift_unit<uint8_t>(p, rows, cols, masks[k] + n * (size_t)b, (uint8_t*)scratch, mask_fill[k], c->stream));
  }
  // the flag grid of the mask (one byte per 64 x 4 cells) is misaligned by the shift: "may hold an untraversable cell" everywhere
  if (c->L.untrav_flags) HIP_TRY(hipMemsetAsync(c->L.untrav_flags, 0x01, untrav_flag_bytes(rows, cols, batch), c->stream));
  c->geo.pos_x = p.info.pos_x;
  c->geo.pos_y = p.info.pos_y;
  c->geo.ax = c->geo.pos_x + (0.5 * c->geo.len_x - 0.5 * c->geo.res);
  c->geo.ay = c->geo.pos_y + (0.5 * c->geo.len_y - 0.5 * c->geo.res);
  drop_graph(c);  // (the geometry is baked into the captured launches)
  // (a context that never received an elevation has no results either way, and the move must not make one up:
  // map_moved(false) is a whole upload, which sets have_elev)
  if (c->st.have_elev() || p.info.results_kept) c->st.map_moved(p.info.results_kept != 0);
  return TE_OK;
}

}  // extern "C"
