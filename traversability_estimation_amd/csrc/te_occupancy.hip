// te_occupancy.hip -- nav_msgs/OccupancyGrid as an output of the device layers: GridMapRosConverter::toOccupancyGrid as the
// reference's visualization config uses it (traversability_estimation/config/visualization/traversability.yaml: four score
// layers, data_min 1.0, data_max 0.0).  The kernel scales, clamps, truncates to int8 and reverses the cell order; one byte per
// cell crosses PCIe.  Semantics: include/travgpu.h; the wire format: te_occupancy.h.
#include "te_ctx.h"
#include "te_occupancy.h"
#include "te_out_kernels.h"

using namespace te;
using namespace te::shim;

namespace te {
namespace occ {
namespace {

// four floats at any float boundary: the groups are aligned for the STORE (below), the loads take what is left
typedef float float4u __attribute__((ext_vector_type(4), aligned(4)));

// toOccupancyGrid for one cell; -ffp-contract=off keeps the operations apart, `/` is the correctly rounded division
__device__ __forceinline__ unsigned cell(float x, float mn, float range) {
  const float v = (x - mn) / range;
  if (v != v) return 0xffu;                // -1
  const float lo = 0.0f < v ? v : 0.0f;    // std::max(0.0f, v)
  const float cl = 1.0f < lo ? 1.0f : lo;  // std::min(.., 1.0f)
  return (unsigned)(int)(0.0f + cl * 100.0f) & 0xffu;
}

// Layer blockIdx.y of the call: cell k of the layer goes to byte (L + 1) * n - 1 - k of `out` (the layers lie back to back,
// each reversed).  A thread reads cells k .. k + 3 and stores them as one dword, last cell in the lowest byte; the groups
// start at k = head so that the dword is aligned: head = ((L + 1) * n) mod 4.  The head cells in front of the first group
// and the up to three behind the last one are stored byte by byte by the first threads of the layer's first block.
__global__ __launch_bounds__(256) void k_occupancy(Job job, size_t n, uint8_t* __restrict__ out) {
  const size_t L = blockIdx.y;
  const Layer ly = job.l[L];
  const size_t last = (L + 1) * n - 1;  // byte of cell 0
  size_t head = ((L + 1) * n) & 3;
  if (head > n) head = n;
  const size_t ngroups = (n - head) >> 2;
  for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += (size_t)gridDim.x * blockDim.x) {
    const size_t k = head + 4 * g;
    const float4u v = *(const float4u*)(ly.src + k);
    const unsigned w = cell(v.w, ly.mn, ly.range) | (cell(v.z, ly.mn, ly.range) << 8) | (cell(v.y, ly.mn, ly.range) << 16) |
                       (cell(v.x, ly.mn, ly.range) << 24);
    *(unsigned*)(out + (last - k - 3)) = w;
  }
  if (blockIdx.x == 0) {
    const size_t tail0 = head + 4 * ngroups;  // first cell behind the groups
    const size_t t = threadIdx.x;
    size_t k = n;
    if (t < head)
      k = t;
    else if (t - head < n - tail0)
      k = tail0 + (t - head);
    if (k < n) out[last - k] = (uint8_t)cell(ly.src[k], ly.mn, ly.range);
  }
}

}  // namespace

hipError_t launch(const Job& job, int n_layers, size_t n, uint8_t* out, hipStream_t stream) {
  const size_t ngroups = n / 4 + 1;
  size_t blocks = (ngroups + 255) / 256;
  if (blocks > 8192) blocks = 8192;  // (grid-stride beyond: 32 blocks per CU)
  hipLaunchKernelGGL(k_occupancy, dim3((unsigned)blocks, (unsigned)n_layers), dim3(256), 0, stream, job, n, out);
  return hipGetLastError();
}

namespace {

// the checks both download calls share and the job of the launch; caller holds the lock
int make_job(const char* who, te_ctx* c, int map, int n_layers, const int* layers, const float* data_min, const float* data_max, Job& job) {
  if (!c->have_geo) return fail(TE_ERR_NOT_READY, "%s: geometry not set", who);
  if (n_layers <= 0 || n_layers > TE_OCCUPANCY_MAX_LAYERS) return fail(TE_ERR_INVALID_ARG, "%s: %d layers (1 .. %d)", who, n_layers, TE_OCCUPANCY_MAX_LAYERS);
  if (map < 0 || map >= c->geo.batch) return fail(TE_ERR_INVALID_ARG, "%s: map %d of batch %d", who, map, c->geo.batch);
  const size_t n = (size_t)c->geo.rows * c->geo.cols;
  memset(&job, 0, sizeof(job));
  for (int k = 0; k < n_layers; ++k) {
    if (!layer_known(c, layers[k])) return fail(TE_ERR_INVALID_ARG, "%s: bad layer %d", who, layers[k]);
    if (!isfinite(data_min[k]) || !isfinite(data_max[k]))
      return fail(TE_ERR_INVALID_ARG, "%s: data_min = %g, data_max = %g", who, (double)data_min[k], (double)data_max[k]);
    const float* p = layer_ptr(c, layers[k]);
    if (!p || (c->user.added(layers[k]) && !(c->st.layers_written() & bit(layers[k])))) return fail(TE_ERR_NOT_READY, "%s: layer %d does not exist yet", who, layers[k]);
    job.l[k].src = p + n * (size_t)map;
    job.l[k].mn = data_min[k];
    job.l[k].range = data_max[k] - data_min[k];
  }
  return TE_OK;
}

// one launch, one transfer; dst: n_layers * rows * cols bytes on the host
int convert_locked(te_ctx* c, const Job& job, int n_layers, void* dst) {
  const size_t n = (size_t)c->geo.rows * c->geo.cols;
  HIP_TRY(hipSetDevice(c->device));
  const size_t bytes = n * (size_t)n_layers;
  HIP_TRY(c->lmem.occ_out.reserve((bytes + 3) & ~(size_t)3, c->stream));
  HIP_TRY(launch(job, n_layers, n, c->lmem.occ_out.as<uint8_t>(), c->stream));
  HIP_TRY(c->stager.download(dst, c->lmem.occ_out.p, bytes, c->stream));  // (returns when dst holds the cells)
  return TE_OK;
}

unsigned layer_bits(int n_layers, const int* layers) {
  unsigned m = 0;
  for (int k = 0; k < n_layers && k < TE_OCCUPANCY_MAX_LAYERS; ++k) m |= bit(layers[k]);
  return m;
}

}  // namespace
}  // namespace occ
}  // namespace te

extern "C" {

int te_download_occupancy(te_ctx* c, int map, int n_layers, const int* layers, const float* data_min, const float* data_max,
                          int8_t* out) {
  if (!c || !layers || !data_min || !data_max || !out) return fail(TE_ERR_INVALID_ARG, "te_download_occupancy: NULL");
  CtxLock lk(c, /*beside_prefetch*/ true, occ::layer_bits(n_layers, layers));
  occ::Job job;
  if (const int rc = occ::make_job("te_download_occupancy", c, map, n_layers, layers, data_min, data_max, job)) return rc;
  return occ::convert_locked(c, job, n_layers, out);
}

int te_download_occupancy_msg(te_ctx* c, const te_msg_info* info, int layer, float data_min, float data_max, void* out, size_t cap,
                              size_t* written) {
  if (!c || !info || !written) return fail(TE_ERR_INVALID_ARG, "te_download_occupancy_msg: NULL");
  CtxLock lk(c, /*beside_prefetch*/ true, bit(layer));
  occ::Job job;  // (every refusal comes before the first byte is written)
  if (const int rc = occ::make_job("te_download_occupancy_msg", c, 0, 1, &layer, &data_min, &data_max, job)) return rc;
  te_occupancy_info oi;
  memset(&oi, 0, sizeof(oi));
  oi.seq = info->seq;
  oi.stamp_sec = oi.map_load_sec = info->stamp_sec;
  oi.stamp_nsec = oi.map_load_nsec = info->stamp_nsec;
  memcpy(oi.frame_id, info->frame_id, sizeof(oi.frame_id));
  oi.resolution = (float)c->geo.res;
  oi.width = (uint32_t)c->geo.rows;
  oi.height = (uint32_t)c->geo.cols;
  oi.origin[0] = c->geo.pos_x - 0.5 * c->geo.len_x;
  oi.origin[1] = c->geo.pos_y - 0.5 * c->geo.len_y;
  oi.origin[6] = 1.0;
  std::string err;
  size_t off = 0;
  *written = 0;
  // size and offset first, then the cells, the header last: a call that fails on the device leaves no valid-looking message
  (void)occ::write_skeleton(oi, nullptr, 0, *written, off, err);  // (*written stays 0 when no buffer would do)
  if (*written == 0 || !out || cap < *written) {
    if (*written) (void)occ::write_skeleton(oi, nullptr, out ? cap : 0, *written, off, err);
    return fail(TE_ERR_INVALID_ARG, "te_download_occupancy_msg: %s", err.c_str());
  }
  if (const int rc = occ::convert_locked(c, job, 1, (uint8_t*)out + off)) return rc;
  if (!occ::write_skeleton(oi, (uint8_t*)out, cap, *written, off, err)) return fail(TE_ERR_INVALID_ARG, "te_download_occupancy_msg: %s", err.c_str());
  return TE_OK;
}

int te_occupancy_msg_write(const te_occupancy_info* info, const int8_t* data, void* out, size_t cap, size_t* written) {
  if (!info || !written) return fail(TE_ERR_INVALID_ARG, "te_occupancy_msg_write: NULL");
  std::string err;
  size_t off = 0;
  *written = 0;
  if (!occ::write_skeleton(*info, (uint8_t*)out, out ? cap : 0, *written, off, err)) return fail(TE_ERR_INVALID_ARG, "te_occupancy_msg_write: %s", err.c_str());
  if (*written > off) {
    if (!data) return fail(TE_ERR_INVALID_ARG, "te_occupancy_msg_write: NULL data");
    memcpy((uint8_t*)out + off, data, *written - off);
  }
  return TE_OK;
}

int te_occupancy_parse(const void* m, size_t len, te_occupancy_info* info, size_t* data_offset) {
  if (!m || !info || !data_offset) return fail(TE_ERR_INVALID_ARG, "te_occupancy_parse: NULL");
  std::string err;
  te_occupancy_info oi;
  size_t off = 0;
  if (!occ::parse((const uint8_t*)m, len, oi, off, err)) return fail(TE_ERR_INVALID_ARG, "te_occupancy_parse: %s", err.c_str());
  *info = oi;
  *data_offset = off;
  return TE_OK;
}

}  // extern "C"
