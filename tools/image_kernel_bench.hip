// image_kernel_bench.hip -- the conversion kernel of te_upload_image (te_image.hip) on its own, against a device-to-device
// copy of one float layer of the same map in the same process: tools/image_upload_bench.py builds and runs it.
//   image_kernel_bench <channels> <bytes_per_channel> [n = 4096] [extra step bytes = 0]
// prints one JSON line: medians of 20 event-timed runs after 3 warm-ups, kernel and copy alternating.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "te_image.h"

#define HIP_OK(expr)                                                                        \
  do {                                                                                      \
    const hipError_t e__ = (expr);                                                          \
    if (e__ != hipSuccess) {                                                                \
      std::fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e__));                      \
      return 1;                                                                             \
    }                                                                                       \
  } while (0)

static float median(std::vector<float> v) {
  std::sort(v.begin(), v.end());
  return 0.5f * (v[(v.size() - 1) / 2] + v[v.size() / 2]);
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: image_kernel_bench <channels> <bytes_per_channel> [n] [extra step bytes]\n");
    return 2;
  }
  te_image_info info = te_image_info();
  info.channels = std::atoi(argv[1]);
  info.bytes_per_channel = std::atoi(argv[2]);
  const int n = argc > 3 ? std::atoi(argv[3]) : 4096;
  info.height = info.width = n;
  info.step = n * info.channels * info.bytes_per_channel + (argc > 4 ? std::atoi(argv[4]) : 0);
  std::string err;
  if (!te::img::check_layout(info, err)) {
    std::fprintf(stderr, "%s\n", err.c_str());
    return 2;
  }
  const size_t bytes = te::img::payload_bytes(info), cells = (size_t)n * n;
  std::vector<uint8_t> host(bytes);
  uint32_t s = 12345;
  for (size_t k = 0; k < bytes; ++k) {  // (about half of the alphas end up below the threshold)
    s = s * 1664525u + 1013904223u;
    host[k] = (uint8_t)(s >> 24);
  }
  void* staged = nullptr;
  float *layer = nullptr, *other = nullptr;
  HIP_OK(hipMalloc(&staged, bytes + te::img::kStagePad));
  HIP_OK(hipMalloc((void**)&layer, cells * sizeof(float)));
  HIP_OK(hipMalloc((void**)&other, cells * sizeof(float)));
  HIP_OK(hipMemcpy(staged, host.data(), bytes, hipMemcpyHostToDevice));
  hipStream_t stream;
  hipEvent_t e0, e1;
  HIP_OK(hipStreamCreate(&stream));
  HIP_OK(hipEventCreate(&e0));
  HIP_OK(hipEventCreate(&e1));
  const unsigned thr = te::img::alpha_threshold_sample(0.5, info.bytes_per_channel);
  const int warmup = 3, iters = 20;
  std::vector<float> t_kernel, t_copy;
  for (int k = 0; k < warmup + iters; ++k) {
    float ms = 0;
    HIP_OK(hipEventRecord(e0, stream));
    HIP_OK(te::img::launch_to_layer(staged, info, layer, 0.0f, 1.0f, thr, stream));
    HIP_OK(hipEventRecord(e1, stream));
    HIP_OK(hipEventSynchronize(e1));
    HIP_OK(hipEventElapsedTime(&ms, e0, e1));
    if (k >= warmup) t_kernel.push_back(ms);
    HIP_OK(hipEventRecord(e0, stream));
    HIP_OK(hipMemcpyDtoDAsync((hipDeviceptr_t)other, (hipDeviceptr_t)layer, cells * sizeof(float), stream));
    HIP_OK(hipEventRecord(e1, stream));
    HIP_OK(hipEventSynchronize(e1));
    HIP_OK(hipEventElapsedTime(&ms, e0, e1));
    if (k >= warmup) t_copy.push_back(ms);
  }
  const float mk = median(t_kernel), mc = median(t_copy);
  const double kernel_bytes = (double)bytes + (double)cells * sizeof(float), copy_bytes = 2.0 * cells * sizeof(float);
  std::printf("{\"n\": %d, \"channels\": %d, \"bytes_per_channel\": %d, \"step\": %d, \"kernel_ms\": %.5f, \"kernel_ms_min\": %.5f, "
              "\"kernel_ms_max\": %.5f, \"copy_ms\": %.5f, \"copy_ms_min\": %.5f, \"copy_ms_max\": %.5f, \"kernel_over_copy\": %.3f, "
              "\"kernel_gb_per_s\": %.1f, \"copy_gb_per_s\": %.1f}\n",
              n, info.channels, info.bytes_per_channel, info.step, mk, *std::min_element(t_kernel.begin(), t_kernel.end()),
              *std::max_element(t_kernel.begin(), t_kernel.end()), mc, *std::min_element(t_copy.begin(), t_copy.end()),
              *std::max_element(t_copy.begin(), t_copy.end()), mk / mc, kernel_bytes / mk * 1e-6, copy_bytes / mc * 1e-6);
  HIP_OK(hipFree(staged));
  HIP_OK(hipFree(layer));
  HIP_OK(hipFree(other));
  return 0;
}
