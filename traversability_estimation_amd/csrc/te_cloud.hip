// te_cloud.hip -- sensor_msgs/PointCloud2 as an output of the device layers: GridMapRosConverter::toPointCloud as the reference's
// visualization config uses it for the elevation layer.  Only the valid cells cross PCIe, in GridMapIterator order.
// Semantics: include/travgpu.h; the wire format and the spans: te_cloud.h.
//
// Order-keeping compaction in three launches on the context's stream, none of which waits for another workgroup:
//   k_cloud_count    workgroup b counts the emitted cells among its kBlockCells cells (ballot + popcount)       -> counts[b]
//   k_cloud_scan     workgroup s owns kScanCounts counts: it sums every count in front of its span, then scans
//                    its own                                                                                     -> offsets[b], offsets[nblocks] = total
//   k_cloud_scatter  workgroup b ballots again and writes the record of its p-th emitted cell at offsets[b] + p
// The scan reads the counts in front of a span once per span: nblocks * nspans / 2 reads of an array that stays in L2
// (4096 x 4096 cells: 32768 counts, 128 spans), in exchange for no flags, no atomics and no fourth launch.
#include "te_cloud.h"
#include "te_ctx.h"
#include "te_geom.h"
#include "te_out_kernels.h"

using namespace te;
using namespace te::shim;

namespace te {
namespace cloud {
namespace {

static_assert(kBlockThreads % kWaveCells == 0 && kScanCounts == kBlockThreads, "one count per scan thread, whole wavefronts");
constexpr int kWaves = kBlockThreads / kWaveCells;
constexpr int kSegments = kWaves * kBlockIters;  // ballots of one workgroup, in cell order

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ bool emitted(const Spec& s, size_t cell, size_t n) {
  if (cell >= n) return false;
  bool ok = finite_f(s.point[cell]);
  for (int k = 0; k < s.n_basic; ++k) ok = ok && finite_f(s.basic[k][cell]);
  return ok;
}

__global__ __launch_bounds__(kBlockThreads) void k_cloud_count(Spec s, size_t n, unsigned* __restrict__ counts) {
  __shared__ unsigned seg[kSegments];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t base = (size_t)blockIdx.x * kBlockCells;
#pragma unroll
  for (int r = 0; r < kBlockIters; ++r) {
    const unsigned long long b = __ballot(emitted(s, base + (size_t)r * kBlockThreads + threadIdx.x, n));
    if (lane == 0) seg[r * kWaves + wave] = (unsigned)__popcll(b);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned c = 0;
#pragma unroll
    for (int k = 0; k < kSegments; ++k) c += seg[k];
    counts[blockIdx.x] = c;
  }
}

// the sum of v over the workgroup's kScanCounts threads, in every thread (red: kWaves slots)
__device__ __forceinline__ unsigned long long block_sum(unsigned long long v, unsigned long long* red) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  __syncthreads();  // (red may still be read from the call before)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long t = 0;
#pragma unroll
  for (int k = 0; k < kWaves; ++k) t += red[k];
  return t;
}

__global__ __launch_bounds__(kScanCounts) void k_cloud_scan(const unsigned* __restrict__ counts, size_t nblocks,
                                                            unsigned long long* __restrict__ offsets) {
  __shared__ unsigned long long red[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t first = (size_t)blockIdx.x * kScanCounts;
  unsigned long long before = 0;
  for (size_t k = threadIdx.x; k < first; k += kScanCounts) before += counts[k];
  before = block_sum(before, red);
  const size_t b = first + threadIdx.x;
  const unsigned long long mine = b < nblocks ? counts[b] : 0;
  // inclusive scan inside the wavefront, then the wavefronts in front
  unsigned long long incl = mine;
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  __syncthreads();
  if (lane == 63) red[wave] = incl;
  __syncthreads();
  unsigned long long front = before;
  for (int k = 0; k < wave; ++k) front += red[k];
  if (b < nblocks) {
    offsets[b] = front + incl - mine;
    if (b == nblocks - 1) offsets[nblocks] = front + incl;
  }
}

__global__ __launch_bounds__(kBlockThreads) void k_cloud_scatter(Spec s, Geo g, size_t n, const unsigned long long* __restrict__ offsets,
                                                                 size_t total, float* __restrict__ out) {
  __shared__ unsigned seg[kSegments];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t base = (size_t)blockIdx.x * kBlockCells;
  bool em[kBlockIters];
  unsigned below[kBlockIters];
#pragma unroll
  for (int r = 0; r < kBlockIters; ++r) {
    em[r] = emitted(s, base + (size_t)r * kBlockThreads + threadIdx.x, n);
    const unsigned long long b = __ballot(em[r]);
    below[r] = (unsigned)__popcll(b & (((unsigned long long)1 << lane) - 1));
    if (lane == 0) seg[r * kWaves + wave] = (unsigned)__popcll(b);
  }
  __syncthreads();
  const unsigned long long first = offsets[blockIdx.x];
#pragma unroll
  for (int r = 0; r < kBlockIters; ++r) {
    if (!em[r]) continue;
    unsigned front = 0;
    for (int k = 0; k < r * kWaves + wave; ++k) front += seg[k];
    const unsigned long long rank = first + front + below[r];
    if (rank >= total) continue;  // (cannot happen while the layers stay as the count saw them: the buffer holds `total` records)
    const size_t cell = base + (size_t)r * kBlockThreads + threadIdx.x;
    const int i = (int)(cell % (size_t)g.rows), j = (int)(cell / (size_t)g.rows);
    float* rec = out + rank * (size_t)s.n_fields;
    for (int f = 0; f < s.n_fields; ++f) {
      float v;
      if (s.kind[f] == kX)
        v = (float)cell_x(g, i);
      else if (s.kind[f] == kY)
        v = (float)cell_y(g, j);
      else
        v = s.field[f][cell];
      rec[f] = v;
    }
  }
}

}  // namespace

size_t n_blocks(size_t n) { return (n + kBlockCells - 1) / kBlockCells; }

hipError_t launch_count_scan(const Spec& s, size_t n, unsigned* counts, unsigned long long* offsets, hipStream_t stream) {
  const size_t nb = n_blocks(n);
  hipLaunchKernelGGL(k_cloud_count, dim3((unsigned)nb), dim3(kBlockThreads), 0, stream, s, n, counts);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_cloud_scan, dim3((unsigned)((nb + kScanCounts - 1) / kScanCounts)), dim3(kScanCounts), 0, stream, counts, nb, offsets);
  return hipGetLastError();
}

hipError_t launch_scatter(const Spec& s, const Geo& g, size_t n, const unsigned long long* offsets, size_t total, float* out,
                          hipStream_t stream) {
  hipLaunchKernelGGL(k_cloud_scatter, dim3((unsigned)n_blocks(n)), dim3(kBlockThreads), 0, stream, s, g, n, offsets, total, out);
  return hipGetLastError();
}

namespace {

// checks the request and fills the spec; caller holds the lock
int make_spec(const char* who, te_ctx* c, int map, int n_layers, const int* layers, int point_layer, int n_basic, const int* basic_layers,
              Spec& s) {
  if (!c->have_geo) return fail(TE_ERR_NOT_READY, "%s: geometry not set", who);
  if (n_layers <= 0 || n_layers > TE_CLOUD_MAX_LAYERS) return fail(TE_ERR_INVALID_ARG, "%s: %d layers (1 .. %d)", who, n_layers, TE_CLOUD_MAX_LAYERS);
  if (n_basic < 0 || n_basic > TE_CLOUD_MAX_LAYERS || (n_basic > 0 && !basic_layers))
    return fail(TE_ERR_INVALID_ARG, "%s: %d basic layers (0 .. %d)", who, n_basic, TE_CLOUD_MAX_LAYERS);
  if (map < 0 || map >= c->geo.batch) return fail(TE_ERR_INVALID_ARG, "%s: map %d of batch %d", who, map, c->geo.batch);
  const size_t at = (size_t)c->geo.rows * c->geo.cols * (size_t)map;
  memset(&s, 0, sizeof(s));
  int seen = 0;
  for (int pass = 0; pass < 2; ++pass) {
    const int m = pass ? n_basic : n_layers;
    const int* ids = pass ? basic_layers : layers;
    for (int k = 0; k < m; ++k) {
      if (!layer_known(c, ids[k])) return fail(TE_ERR_INVALID_ARG, "%s: bad layer %d", who, ids[k]);
      const float* p = layer_ptr(c, ids[k]);
      if (!p || (c->user.added(ids[k]) && !(c->st.layers_written() & bit(ids[k])))) return fail(TE_ERR_NOT_READY, "%s: layer %d does not exist yet", who, ids[k]);
      if (pass) {
        s.basic[k] = p + at;
      } else if (ids[k] == point_layer) {
        if (++seen > 1) break;
        s.kind[s.n_fields++] = kX;
        s.kind[s.n_fields++] = kY;
        s.point = p + at;
        s.field[s.n_fields++] = p + at;
      } else {
        s.field[s.n_fields++] = p + at;
      }
    }
  }
  if (seen != 1) return fail(TE_ERR_INVALID_ARG, "%s: the point layer %d appears %s in the layers", who, point_layer, seen ? "more than once" : "nowhere");
  s.n_basic = n_basic;
  return TE_OK;
}

// launches 1 and 2 and the small copy: the number of points
int count_points(te_ctx* c, const Spec& s, size_t& total) {
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = (size_t)c->geo.rows * c->geo.cols, nb = n_blocks(n);
  const size_t counts_bytes = (nb * sizeof(unsigned) + 7) & ~(size_t)7;
  HIP_TRY(c->lmem.cloud_counts.reserve(counts_bytes + (nb + 1) * sizeof(unsigned long long), c->stream));
  unsigned* counts = c->lmem.cloud_counts.as<unsigned>();
  unsigned long long* offsets = (unsigned long long*)(c->lmem.cloud_counts.as<char>() + counts_bytes);
  HIP_TRY(launch_count_scan(s, n, counts, offsets, c->stream));
  unsigned long long t = 0;
  HIP_TRY(hipMemcpyAsync(&t, offsets + nb, sizeof(t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  total = (size_t)t;
  return TE_OK;
}

// launch 3 and the transfer of total records into dst (host); count_points has run
int scatter_points(te_ctx* c, const Spec& s, size_t total, void* dst) {
  if (total == 0) return TE_OK;
  const size_t n = (size_t)c->geo.rows * c->geo.cols, nb = n_blocks(n);
  const size_t counts_bytes = (nb * sizeof(unsigned) + 7) & ~(size_t)7;
  const unsigned long long* offsets = (const unsigned long long*)(c->lmem.cloud_counts.as<char>() + counts_bytes);
  const size_t bytes = total * (size_t)s.n_fields * sizeof(float);
  HIP_TRY(c->lmem.cloud_out.reserve(bytes, c->stream));
  HIP_TRY(launch_scatter(s, c->geo, n, offsets, total, c->lmem.cloud_out.as<float>(), c->stream));
  HIP_TRY(c->stager.download(dst, c->lmem.cloud_out.p, bytes, c->stream));  // (returns when dst holds the records)
  return TE_OK;
}

unsigned layer_bits(int n, const int* ids) {
  unsigned m = 0;
  for (int k = 0; ids && k < n && k < TE_CLOUD_MAX_LAYERS; ++k) m |= bit(ids[k]);
  return m;
}

}  // namespace
}  // namespace cloud
}  // namespace te

extern "C" {

int te_download_cloud(te_ctx* c, int map, int n_layers, const int* layers, int point_layer, int n_basic, const int* basic_layers, float* out,
                      size_t cap_points, size_t* n_points) {
  if (!c || !layers || !n_points || (!out && cap_points)) return fail(TE_ERR_INVALID_ARG, "te_download_cloud: NULL");
  CtxLock lk(c, /*beside_prefetch*/ true, cloud::layer_bits(n_layers, layers) | cloud::layer_bits(n_basic, basic_layers));
  cloud::Spec s;
  if (const int rc = cloud::make_spec("te_download_cloud", c, map, n_layers, layers, point_layer, n_basic, basic_layers, s)) return rc;
  size_t total = 0;
  if (const int rc = cloud::count_points(c, s, total)) return rc;
  *n_points = total;
  if (!out && !cap_points) return TE_OK;  // the sizing call
  if (total > cap_points) return fail(TE_ERR_INVALID_ARG, "te_download_cloud: %zu points, room for %zu", total, cap_points);
  return cloud::scatter_points(c, s, total, out);
}

int te_download_cloud_msg(te_ctx* c, const te_msg_info* info, int n_layers, const int* layers, const char* const* names, int point_layer,
                          int n_basic, const int* basic_layers, void* out, size_t cap, size_t* written) {
  if (!c || !info || !layers || !names || !written) return fail(TE_ERR_INVALID_ARG, "te_download_cloud_msg: NULL");
  CtxLock lk(c, /*beside_prefetch*/ true, cloud::layer_bits(n_layers, layers) | cloud::layer_bits(n_basic, basic_layers));
  cloud::Spec s;
  if (const int rc = cloud::make_spec("te_download_cloud_msg", c, 0, n_layers, layers, point_layer, n_basic, basic_layers, s)) return rc;
  const char* fields[TE_CLOUD_MAX_LAYERS + 2];
  int nf = 0;
  for (int k = 0; k < n_layers; ++k) {
    if (layers[k] == point_layer) {
      fields[nf++] = "x";
      fields[nf++] = "y";
      fields[nf++] = "z";
    } else {
      if (!names[k]) return fail(TE_ERR_INVALID_ARG, "te_download_cloud_msg: NULL name");
      if (strlen(names[k]) >= TE_MSG_MAX_NAME) return fail(TE_ERR_INVALID_ARG, "te_download_cloud_msg: field name longer than %d", TE_MSG_MAX_NAME - 1);
      fields[nf++] = names[k];
    }
  }
  size_t total = 0;
  if (const int rc = cloud::count_points(c, s, total)) return rc;
  if (total > 0xffffffffull) return fail(TE_ERR_INVALID_ARG, "te_download_cloud_msg: %zu points do not fit a message", total);
  te_cloud_info ci;
  memset(&ci, 0, sizeof(ci));
  ci.seq = info->seq;
  ci.stamp_sec = info->stamp_sec;
  ci.stamp_nsec = info->stamp_nsec;
  memcpy(ci.frame_id, info->frame_id, sizeof(ci.frame_id));
  ci.width = (uint32_t)total;
  ci.is_dense = 0;
  std::string err;
  size_t off = 0;
  *written = 0;
  // size and offset first, then the points, the header last: a call that fails on the device leaves no valid-looking message
  (void)cloud::write_skeleton(ci, cloud::Names{nf, fields}, nullptr, 0, *written, off, err);  // (*written stays 0 when no buffer would do)
  if (*written == 0 || !out || cap < *written) {
    if (*written) (void)cloud::write_skeleton(ci, cloud::Names{nf, fields}, nullptr, out ? cap : 0, *written, off, err);
    return fail(TE_ERR_INVALID_ARG, "te_download_cloud_msg: %s", err.c_str());
  }
  if (const int rc = cloud::scatter_points(c, s, total, (uint8_t*)out + off)) return rc;
  if (!cloud::write_skeleton(ci, cloud::Names{nf, fields}, (uint8_t*)out, cap, *written, off, err))
    return fail(TE_ERR_INVALID_ARG, "te_download_cloud_msg: %s", err.c_str());
  return TE_OK;
}

int te_cloud_msg_write(const te_cloud_info* info, int n_fields, const char* const* field_names, const float* points, void* out, size_t cap,
                       size_t* written) {
  if (!info || !written || !field_names) return fail(TE_ERR_INVALID_ARG, "te_cloud_msg_write: NULL");
  std::string err;
  size_t off = 0;
  *written = 0;
  if (!cloud::write_skeleton(*info, cloud::Names{n_fields, field_names}, (uint8_t*)out, out ? cap : 0, *written, off, err))
    return fail(TE_ERR_INVALID_ARG, "te_cloud_msg_write: %s", err.c_str());
  const size_t bytes = (size_t)info->width * 4 * (size_t)n_fields;
  if (bytes) {
    if (!points) return fail(TE_ERR_INVALID_ARG, "te_cloud_msg_write: NULL points");
    memcpy((uint8_t*)out + off, points, bytes);
  }
  return TE_OK;
}

int te_cloud_parse(const void* m, size_t len, te_cloud_info* info, size_t* data_offset) {
  if (!m || !info || !data_offset) return fail(TE_ERR_INVALID_ARG, "te_cloud_parse: NULL");
  std::string err;
  te_cloud_info ci;
  size_t off = 0;
  if (!cloud::parse((const uint8_t*)m, len, ci, off, nullptr, err)) return fail(TE_ERR_INVALID_ARG, "te_cloud_parse: %s", err.c_str());
  *info = ci;
  *data_offset = off;
  return TE_OK;
}

int te_cloud_field(const void* m, size_t len, int k, char* name, uint32_t* offset, uint32_t* datatype, uint32_t* count) {
  if (!m || !name || !offset || !datatype || !count) return fail(TE_ERR_INVALID_ARG, "te_cloud_field: NULL");
  std::string err;
  te_cloud_info ci;
  size_t off = 0;
  std::vector<cloud::FieldView> fv;
  if (!cloud::parse((const uint8_t*)m, len, ci, off, &fv, err)) return fail(TE_ERR_INVALID_ARG, "te_cloud_field: %s", err.c_str());
  if (k < 0 || k >= (int)fv.size()) return fail(TE_ERR_INVALID_ARG, "te_cloud_field: field %d of %zu", k, fv.size());
  memcpy(name, fv[k].name, fv[k].name_len);  // (shorter than TE_MSG_MAX_NAME: the parser checked)
  name[fv[k].name_len] = 0;
  *offset = fv[k].offset;
  *datatype = fv[k].datatype;
  *count = fv[k].count;
  return TE_OK;
}

int te_cloud_spans(size_t cells[3]) {
  if (!cells) return fail(TE_ERR_INVALID_ARG, "te_cloud_spans: NULL");
  cells[0] = cloud::kWaveCells;
  cells[1] = cloud::kBlockCells;
  cells[2] = cloud::kScanCells;
  return TE_OK;
}

}  // extern "C"
