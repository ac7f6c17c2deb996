// te_submap.hip -- the data path behind the reference's get_traversability service (TraversabilityEstimation.cpp:297-316):
// GridMap::getSubmap(position, length) of the resident map, the requested layers only.  The rectangle comes from
// te_submap_plan.h; one kernel packs it out of up to 16 layers into one buffer, which crosses PCIe in one transfer.
// Semantics: include/travgpu.h.
#include "te_ctx.h"
#include "te_out_kernels.h"
#include "te_submap_plan.h"

using namespace te;
using namespace te::shim;

namespace te {
namespace submap {
namespace {

// four floats at any float boundary: the groups are aligned for the STORE (below), the loads take what is left
typedef float float4u __attribute__((ext_vector_type(4), aligned(4)));
typedef float float4a __attribute__((ext_vector_type(4), aligned(16)));

constexpr int kLanes = 64;  // threads along a column: one 16-byte group each
constexpr int kCols = 4;    // columns of a workgroup

// Layer blockIdx.z of the call: column j of the h x w rectangle -- h floats at src + j * stride -- goes to the h floats at
// out + (L * w + j) * h.  Source columns are stride * 4 bytes apart and destination columns h * 4 bytes, so the 16-byte
// alignment of either changes from column to column.  A column is cut for its DESTINATION: `head` floats up to the first
// 16-byte boundary of the destination, then groups of four -- one 16-byte load at whatever alignment the source has there,
// one aligned 16-byte store -- then up to three floats behind the last group.  Slot g of a column is group g; the two slots
// behind the largest possible group count copy the head and the tail float by float.  The values move as bits.
__global__ __launch_bounds__(kLanes* kCols) void k_submap_pack(Job job, size_t stride, int h, int w, float* __restrict__ out) {
  const float* __restrict__ src = job.src[blockIdx.z];
  float* const dst = out + (size_t)blockIdx.z * (size_t)w * (size_t)h;
  const long long slots = (long long)(h >> 2) + 2;
  for (long long j = (long long)blockIdx.y * kCols + threadIdx.y; j < w; j += (long long)gridDim.y * kCols) {
    const float* s = src + (size_t)j * stride;
    float* d = dst + (size_t)j * (size_t)h;
    int head = (int)(((16u - (unsigned)((uintptr_t)d & 15u)) & 15u) >> 2);
    if (head > h) head = h;
    const int ngroups = (h - head) >> 2;
    for (long long g = (long long)blockIdx.x * kLanes + threadIdx.x; g < slots; g += (long long)gridDim.x * kLanes) {
      if (g < ngroups) {
        const size_t k = (size_t)head + 4 * (size_t)g;
        *(float4a*)(d + k) = *(const float4u*)(s + k);
      } else if (g == slots - 2) {
        for (int k = 0; k < head; ++k) d[k] = s[k];
      } else if (g == slots - 1) {
        for (int k = head + 4 * ngroups; k < h; ++k) d[k] = s[k];
      }
    }
  }
}

}  // namespace

hipError_t launch(const Job& job, int n_layers, size_t stride, int h, int w, float* out, hipStream_t stream) {
  const long long slots = (long long)(h >> 2) + 2;
  long long bx = (slots + kLanes - 1) / kLanes, by = ((long long)w + kCols - 1) / kCols;
  if (bx > 1024) bx = 1024;  // (grid-stride beyond, both ways)
  if (by > 4096) by = 4096;
  hipLaunchKernelGGL(k_submap_pack, dim3((unsigned)bx, (unsigned)by, (unsigned)n_layers), dim3(kLanes, kCols), 0, stream, job, stride, h, w,
                     out);
  return hipGetLastError();
}

namespace {

unsigned layer_bits(int n_layers, const int* layers) {
  unsigned m = 0;
  for (int k = 0; layers && k < n_layers && k < TE_SUBMAP_MAX_LAYERS; ++k) m |= bit(layers[k]);
  return m;
}

// the checks both calls share, the plan of the request and the job of the launch; caller holds the lock
int make_job(const char* who, te_ctx* c, int map, double req_x, double req_y, double req_len_x, double req_len_y, int n_layers,
             const int* layers, te_submap_info& si, Job& job) {
  si = te_submap_info();
  if (!c->have_geo) return fail(TE_ERR_NOT_READY, "%s: geometry not set", who);
  if (n_layers <= 0 || n_layers > TE_SUBMAP_MAX_LAYERS) return fail(TE_ERR_INVALID_ARG, "%s: %d layers (1 .. %d)", who, n_layers, TE_SUBMAP_MAX_LAYERS);
  if (map < 0 || map >= c->geo.batch) return fail(TE_ERR_INVALID_ARG, "%s: map %d of batch %d", who, map, c->geo.batch);
  const char* why = "";
  if (const int rc = plan(c->geo.rows, c->geo.cols, c->geo.res, c->geo.pos_x, c->geo.pos_y, req_x, req_y, req_len_x, req_len_y, &si, &why))
    return fail(rc, "%s: %s", who, why);
  const size_t n = (size_t)c->geo.rows * c->geo.cols;
  memset(&job, 0, sizeof(job));
  for (int k = 0; k < n_layers; ++k) {
    float* p = nullptr;  // (as te_download_msg: no such id, or a layer that does not exist yet)
    if (const int rc = readable_layer(who, c, layers[k], &p)) return rc;
    job.src[k] = p + n * (size_t)map;
  }
  if (!si.ok) return TE_OK;
  // the kernel reads and writes by the plan without a bounds check of its own: the rectangle lies in the map, or nothing runs
  if (si.row0 < 0 || si.col0 < 0 || si.rows < 1 || si.cols < 1 || si.rows > c->geo.rows - si.row0 || si.cols > c->geo.cols - si.col0)
    return fail(TE_ERR_INVALID_ARG, "%s: the submap (%d,%d)+(%d,%d) leaves the %dx%d map", who, si.row0, si.col0, si.rows, si.cols, c->geo.rows,
                c->geo.cols);
  for (int k = 0; k < n_layers; ++k) job.src[k] += (size_t)si.col0 * c->geo.rows + si.row0;
  return TE_OK;
}

// one launch, one transfer; dst: n_layers * si.rows * si.cols floats on the host
int pack_locked(te_ctx* c, const Job& job, int n_layers, const te_submap_info& si, void* dst) {
  HIP_TRY(hipSetDevice(c->device));
  Carve cv;
  const auto p_out = cv.add<float>((size_t)n_layers * si.rows * si.cols);
  DevBuf tmp;  // (freed when the call returns: the transfer below has been waited for)
  HIP_TRY(tmp.once(cv.total));
  HIP_TRY(launch(job, n_layers, (size_t)c->geo.rows, si.rows, si.cols, p_out.in(tmp), c->stream));
  HIP_TRY(c->stager.download(dst, p_out.in(tmp), p_out.bytes(), c->stream));  // (returns when dst holds the cells)
  return TE_OK;
}

}  // namespace
}  // namespace submap
}  // namespace te

extern "C" {

int te_submap_geometry(int rows, int cols, double resolution, double pos_x, double pos_y, double req_x, double req_y, double req_len_x,
                       double req_len_y, te_submap_info* out) {
  if (!out) return fail(TE_ERR_INVALID_ARG, "te_submap_geometry: NULL");
  const char* why = "";
  if (const int rc = submap::plan(rows, cols, resolution, pos_x, pos_y, req_x, req_y, req_len_x, req_len_y, out, &why))
    return fail(rc, "te_submap_geometry: %s", why);
  return TE_OK;
}

int te_download_submap(te_ctx* c, int map, double req_x, double req_y, double req_len_x, double req_len_y, int n_layers, const int* layers,
                       te_submap_info* info, float* out, size_t cap_floats) {
  if (!c || !layers || !info || (!out && cap_floats)) return fail(TE_ERR_INVALID_ARG, "te_download_submap: NULL");
  CtxLock lk(c, /*beside_prefetch*/ true, submap::layer_bits(n_layers, layers));
  submap::Job job;
  if (const int rc = submap::make_job("te_download_submap", c, map, req_x, req_y, req_len_x, req_len_y, n_layers, layers, *info, job)) return rc;
  if (!info->ok) return TE_OK;  // (the service's isSuccess = false: no map)
  const size_t need = (size_t)n_layers * info->rows * info->cols;
  if (need > cap_floats) return fail(TE_ERR_INVALID_ARG, "te_download_submap: %zu floats, room for %zu", need, cap_floats);
  return submap::pack_locked(c, job, n_layers, *info, out);
}

int te_download_submap_msg(te_ctx* c, const te_msg_info* info_in, double req_x, double req_y, double req_len_x, double req_len_y, int n_layers,
                           const int* layers, const char* const* names, int n_basic, const char* const* basic_names, te_submap_info* info,
                           void* out, size_t cap, size_t* written) {
  if (!c || !info_in || !layers || !names || !info || !written) return fail(TE_ERR_INVALID_ARG, "te_download_submap_msg: NULL");
  *written = 0;
  CtxLock lk(c, /*beside_prefetch*/ true, submap::layer_bits(n_layers, layers));
  submap::Job job;  // (every refusal comes before the first byte is written)
  if (const int rc = submap::make_job("te_download_submap_msg", c, 0, req_x, req_y, req_len_x, req_len_y, n_layers, layers, *info, job)) return rc;
  if (!info->ok) return TE_OK;
  // toMessage(subMap, layers): the submap's own geometry, start index (0, 0)
  te_msg_info mi = *info_in;
  mi.rows = info->rows;
  mi.cols = info->cols;
  mi.resolution = c->geo.res;
  mi.length_x = info->length_x;
  mi.length_y = info->length_y;
  mi.pose[0] = info->pos_x;
  mi.pose[1] = info->pos_y;
  mi.start_row = mi.start_col = 0;
  const msg::Names ln = {n_layers, names}, bn = {n_basic, basic_names};
  *written = msg::message_size(mi, ln, bn);
  std::vector<size_t> off;
  std::string err;
  // size and offsets first (nothing is written: no buffer is passed), then the cells, the header last: a call that fails on the
  // device leaves no valid-looking message
  if (!msg::write_skeleton(mi, ln, bn, nullptr, (size_t)-1, off, err)) return fail(TE_ERR_INVALID_ARG, "te_download_submap_msg: %s", err.c_str());
  if (!out || cap < *written) return fail(TE_ERR_INVALID_ARG, "te_download_submap_msg: grid map message: output buffer too small");
  // The packed buffer lands where the first payload starts, in one transfer; the layers behind the first then move up to
  // their own offsets, last one first (every one moves towards the end of the buffer, past nothing that is still to move).
  const size_t layer_bytes = (size_t)info->rows * info->cols * sizeof(float);
  uint8_t* const o = (uint8_t*)out;
  if (const int rc = submap::pack_locked(c, job, n_layers, *info, o + off[0])) return rc;
  for (int k = n_layers - 1; k > 0; --k) memmove(o + off[k], o + off[0] + (size_t)k * layer_bytes, layer_bytes);
  if (!msg::write_skeleton(mi, ln, bn, o, cap, off, err)) return fail(TE_ERR_INVALID_ARG, "te_download_submap_msg: %s", err.c_str());
  return TE_OK;
}

}  // extern "C"
