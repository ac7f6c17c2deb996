// output_kernel_bench.hip -- the kernels of te_download_occupancy (te_occupancy.hip) and te_download_cloud (te_cloud.hip) on
// their own, against a device-to-device copy of one float layer of the same map in the same process; linked against
// libtravgpu.so (te_out_kernels.h), built and run by tools/output_bench.py.
//   output_kernel_bench occupancy <layers> [n = 4096]
//   output_kernel_bench cloud <holes in percent> [n = 4096]
// prints one JSON line: medians (and min, max) of 20 event-timed runs after 3 warm-ups, the candidates taking turns.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "te_out_kernels.h"

#define HIP_OK(expr)                                                   \
  do {                                                                 \
    const hipError_t e__ = (expr);                                     \
    if (e__ != hipSuccess) {                                           \
      std::fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e__)); \
      return 1;                                                        \
    }                                                                  \
  } while (0)

struct Stat {
  std::vector<float> v;
  float median() {
    std::sort(v.begin(), v.end());
    return 0.5f * (v[(v.size() - 1) / 2] + v[v.size() / 2]);
  }
  void print(const char* name) { std::printf("\"%s_ms\": %.4f, \"%s_min_ms\": %.4f, \"%s_max_ms\": %.4f", name, median(), name, v.front(), name, v.back()); }
};

int main(int argc, char** argv) {
  if (argc < 3 || (std::strcmp(argv[1], "occupancy") != 0 && std::strcmp(argv[1], "cloud") != 0)) {
    std::fprintf(stderr, "usage: output_kernel_bench occupancy <layers> [n] | cloud <holes in percent> [n]\n");
    return 2;
  }
  const bool cloud = std::strcmp(argv[1], "cloud") == 0;
  const int arg = std::atoi(argv[2]);
  const int n = argc > 3 ? std::atoi(argv[3]) : 4096;
  const int n_layers = cloud ? 1 : arg;
  if (n <= 0 || n_layers < 1 || n_layers > TE_OCCUPANCY_MAX_LAYERS || arg < 0 || arg > 100) return 2;
  const size_t cells = (size_t)n * n;
  const int warmup = 3, iters = 20;
  std::vector<float> host(cells);
  std::vector<float*> layer(n_layers);
  uint32_t s = 12345;
  for (int l = 0; l < n_layers; ++l) {
    for (size_t k = 0; k < cells; ++k) {
      s = s * 1664525u + 1013904223u;
      host[k] = (float)(s >> 8) * (1.0f / 16777216.0f);
      if (cloud && (int)((s >> 4) % 100u) < arg) host[k] = NAN;
    }
    HIP_OK(hipMalloc((void**)&layer[l], cells * sizeof(float)));
    HIP_OK(hipMemcpy(layer[l], host.data(), cells * sizeof(float), hipMemcpyHostToDevice));
  }
  float* other = nullptr;
  HIP_OK(hipMalloc((void**)&other, cells * sizeof(float)));
  hipStream_t stream;
  hipEvent_t e0, e1;
  HIP_OK(hipStreamCreate(&stream));
  HIP_OK(hipEventCreate(&e0));
  HIP_OK(hipEventCreate(&e1));
  Stat copy, kern, count_scan, scatter;
  float ms = 0.0f;
  size_t total = 0;
  if (!cloud) {
    te::occ::Job job;
    std::memset(&job, 0, sizeof(job));
    for (int l = 0; l < n_layers; ++l) job.l[l] = te::occ::Layer{layer[l], 1.0f, -1.0f};  // data_min 1, data_max 0
    uint8_t* out = nullptr;
    HIP_OK(hipMalloc((void**)&out, cells * n_layers + 4));
    for (int k = 0; k < warmup + iters; ++k) {
      HIP_OK(hipEventRecord(e0, stream));
      HIP_OK(te::occ::launch(job, n_layers, cells, out, stream));
      HIP_OK(hipEventRecord(e1, stream));
      HIP_OK(hipEventSynchronize(e1));
      HIP_OK(hipEventElapsedTime(&ms, e0, e1));
      if (k >= warmup) kern.v.push_back(ms);
      HIP_OK(hipEventRecord(e0, stream));
      HIP_OK(hipMemcpyDtoDAsync((hipDeviceptr_t)other, (hipDeviceptr_t)layer[0], cells * sizeof(float), stream));
      HIP_OK(hipEventRecord(e1, stream));
      HIP_OK(hipEventSynchronize(e1));
      HIP_OK(hipEventElapsedTime(&ms, e0, e1));
      if (k >= warmup) copy.v.push_back(ms);
    }
  } else {
    te::cloud::Spec spec;
    std::memset(&spec, 0, sizeof(spec));
    spec.kind[0] = te::cloud::kX;
    spec.kind[1] = te::cloud::kY;
    spec.field[2] = spec.point = layer[0];
    spec.n_fields = 3;
    te::Geo g;
    std::memset(&g, 0, sizeof(g));
    g.rows = g.cols = n;
    g.batch = 1;
    g.res = 0.05;
    g.len_x = g.len_y = n * 0.05;
    g.ax = g.ay = 0.5 * g.len_x - 0.5 * g.res;
    const size_t nb = te::cloud::n_blocks(cells);
    unsigned* counts = nullptr;
    unsigned long long* offsets = nullptr;
    float* out = nullptr;
    HIP_OK(hipMalloc((void**)&counts, nb * sizeof(unsigned)));
    HIP_OK(hipMalloc((void**)&offsets, (nb + 1) * sizeof(unsigned long long)));
    HIP_OK(hipMalloc((void**)&out, cells * 3 * sizeof(float)));
    for (int k = 0; k < warmup + iters; ++k) {
      HIP_OK(hipEventRecord(e0, stream));
      HIP_OK(te::cloud::launch_count_scan(spec, cells, counts, offsets, stream));
      HIP_OK(hipEventRecord(e1, stream));
      HIP_OK(hipEventSynchronize(e1));
      HIP_OK(hipEventElapsedTime(&ms, e0, e1));
      if (k >= warmup) count_scan.v.push_back(ms);
      unsigned long long t = 0;
      HIP_OK(hipMemcpy(&t, offsets + nb, sizeof(t), hipMemcpyDeviceToHost));
      total = (size_t)t;
      HIP_OK(hipEventRecord(e0, stream));
      HIP_OK(te::cloud::launch_scatter(spec, g, cells, offsets, total, out, stream));
      HIP_OK(hipEventRecord(e1, stream));
      HIP_OK(hipEventSynchronize(e1));
      HIP_OK(hipEventElapsedTime(&ms, e0, e1));
      if (k >= warmup) scatter.v.push_back(ms);
      HIP_OK(hipEventRecord(e0, stream));
      HIP_OK(hipMemcpyDtoDAsync((hipDeviceptr_t)other, (hipDeviceptr_t)layer[0], cells * sizeof(float), stream));
      HIP_OK(hipEventRecord(e1, stream));
      HIP_OK(hipEventSynchronize(e1));
      HIP_OK(hipEventElapsedTime(&ms, e0, e1));
      if (k >= warmup) copy.v.push_back(ms);
    }
  }
  std::printf("{\"what\": \"%s\", \"arg\": %d, \"n\": %d, ", argv[1], arg, n);
  if (!cloud) {
    kern.print("kernel");
    std::printf(", \"kernel_mb\": %.1f, ", (double)cells * n_layers * 5.0 / 1e6);
  } else {
    count_scan.print("count_scan");
    std::printf(", ");
    scatter.print("scatter");
    std::printf(", \"points\": %zu, \"kernels_mb\": %.1f, ", total, ((double)cells * 8.0 + (double)total * 12.0) / 1e6);
  }
  copy.print("layer_copy");
  std::printf("}\n");
  return 0;
}
