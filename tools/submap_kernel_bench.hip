// submap_kernel_bench.hip -- the pack kernel of te_download_submap (te_submap.hip) on its own, against a device-to-device copy
// of the same bytes in the same process; linked against libtravgpu.so (te_out_kernels.h), built and run by
// tools/submap_bench.py.
//   submap_kernel_bench <layers> [n = 4096] [h = 167] [w = 167]
// the h x w rectangle in the middle of n x n layers.  Prints one JSON line: medians (and min, max) of 30 event-timed runs
// after 5 warm-ups, the candidates taking turns.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
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
  if (argc < 2) {
    std::fprintf(stderr, "usage: submap_kernel_bench <layers> [n] [h] [w]\n");
    return 2;
  }
  const int n_layers = std::atoi(argv[1]);
  const int n = argc > 2 ? std::atoi(argv[2]) : 4096;
  const int h = argc > 3 ? std::atoi(argv[3]) : 167, w = argc > 4 ? std::atoi(argv[4]) : 167;
  if (n_layers < 1 || n_layers > TE_SUBMAP_MAX_LAYERS || n <= 0 || h < 1 || w < 1 || h > n || w > n) return 2;
  const size_t cells = (size_t)n * n, sub = (size_t)h * w * n_layers;
  const int warmup = 5, iters = 30;
  const int row0 = (n - h) / 2 | 1, col0 = (n - w) / 2;  // (an odd first row where there is room: no column starts on a 16-byte boundary)
  std::vector<float> host(cells);
  te::submap::Job job;
  std::memset(&job, 0, sizeof(job));
  uint32_t s = 12345;
  for (int l = 0; l < n_layers; ++l) {
    for (size_t k = 0; k < cells; ++k) {
      s = s * 1664525u + 1013904223u;
      host[k] = (float)(s >> 8) * (1.0f / 16777216.0f);
    }
    float* layer = nullptr;
    HIP_OK(hipMalloc((void**)&layer, cells * sizeof(float)));
    HIP_OK(hipMemcpy(layer, host.data(), cells * sizeof(float), hipMemcpyHostToDevice));
    job.src[l] = layer + (size_t)col0 * n + (row0 + h <= n ? row0 : 0);
  }
  float *out = nullptr, *other = nullptr;
  HIP_OK(hipMalloc((void**)&out, sub * sizeof(float)));
  HIP_OK(hipMalloc((void**)&other, sub * sizeof(float)));
  hipStream_t stream;
  hipEvent_t e0, e1;
  HIP_OK(hipStreamCreate(&stream));
  HIP_OK(hipEventCreate(&e0));
  HIP_OK(hipEventCreate(&e1));
  Stat copy, kern;
  float ms = 0.0f;
  for (int k = 0; k < warmup + iters; ++k) {
    HIP_OK(hipEventRecord(e0, stream));
    HIP_OK(te::submap::launch(job, n_layers, (size_t)n, h, w, out, stream));
    HIP_OK(hipEventRecord(e1, stream));
    HIP_OK(hipEventSynchronize(e1));
    HIP_OK(hipEventElapsedTime(&ms, e0, e1));
    if (k >= warmup) kern.v.push_back(ms);
    HIP_OK(hipEventRecord(e0, stream));
    HIP_OK(hipMemcpyDtoDAsync((hipDeviceptr_t)other, (hipDeviceptr_t)out, sub * sizeof(float), stream));
    HIP_OK(hipEventRecord(e1, stream));
    HIP_OK(hipEventSynchronize(e1));
    HIP_OK(hipEventElapsedTime(&ms, e0, e1));
    if (k >= warmup) copy.v.push_back(ms);
  }
  // the packed buffer against the rectangle of the first and the last layer, on the host
  std::vector<float> got(sub), col(h);
  HIP_OK(hipMemcpy(got.data(), out, sub * sizeof(float), hipMemcpyDeviceToHost));
  int bad = 0;
  for (int l : {0, n_layers - 1})
    for (int j = 0; j < w; ++j) {
      HIP_OK(hipMemcpy(col.data(), job.src[l] + (size_t)j * n, (size_t)h * sizeof(float), hipMemcpyDeviceToHost));
      bad += std::memcmp(col.data(), &got[((size_t)l * w + j) * h], (size_t)h * sizeof(float)) != 0;
    }
  if (bad) {
    std::fprintf(stderr, "%d columns of the packed buffer differ from the layers\n", bad);
    return 1;
  }
  std::printf("{\"layers\": %d, \"n\": %d, \"h\": %d, \"w\": %d, ", n_layers, n, h, w);
  kern.print("kernel");
  std::printf(", \"kernel_kb\": %.1f, ", (double)sub * 8.0 / 1e3);  // read + written
  copy.print("copy_same_bytes");
  std::printf("}\n");
  return 0;
}
