// te_out_kernels.h -- the launches of the two output conversions (te_occupancy.hip, te_cloud.hip) and of the submap pack
// (te_submap.hip) as the entry points and tools/output_kernel_bench.hip / tools/submap_kernel_bench.hip call them: plain device
// pointers, one stream, no context.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "te_internal.h"
#include "travgpu.h"

namespace te {
namespace occ {

struct Layer {
  const float* src;  // the n cells of one map of a layer
  float mn, range;   // data_min, data_max - data_min (float32, rounded once)
};
struct Job {
  Layer l[TE_OCCUPANCY_MAX_LAYERS];
};
// layers 0 .. n_layers - 1 of `job`, n cells each -> out[k * n ..), each reversed; out: 4-byte aligned, n_layers * n bytes.
// One launch.
hipError_t launch(const Job& job, int n_layers, size_t n, uint8_t* out, hipStream_t stream);

}  // namespace occ

namespace cloud {

enum FieldKind { kValue = 0, kX = 1, kY = 2 };
struct Spec {
  const float* field[TE_CLOUD_MAX_LAYERS + 2];  // one map of a layer (kValue; z is the point layer's), unused for kX / kY
  int kind[TE_CLOUD_MAX_LAYERS + 2];
  int n_fields;
  const float* point;                       // the point layer
  const float* basic[TE_CLOUD_MAX_LAYERS];  // GridMap::isValid(index, basicLayers)
  int n_basic;
};
// workgroups of the count and scatter kernels for n cells; the scratch of a map: counts[n_blocks], offsets[n_blocks + 1]
size_t n_blocks(size_t n);
// launches 1 and 2: offsets[b] = emitted cells in front of workgroup b, offsets[n_blocks] = their total
hipError_t launch_count_scan(const Spec& s, size_t n, unsigned* counts, unsigned long long* offsets, hipStream_t stream);
// launch 3: the records of the `total` emitted cells into out (total * n_fields floats)
hipError_t launch_scatter(const Spec& s, const Geo& g, size_t n, const unsigned long long* offsets, size_t total, float* out,
                          hipStream_t stream);

}  // namespace cloud

namespace submap {

struct Job {
  const float* src[TE_SUBMAP_MAX_LAYERS];  // cell (row0, col0) of one map of a layer: the rectangle's first cell
};
// the h x w rectangles of layers 0 .. n_layers - 1 of `job` (columns `stride` floats apart) -> out[(k * w + j) * h + i]: the
// column-major h x w matrices one after another; out: any float boundary, n_layers * w * h floats.  One launch.
hipError_t launch(const Job& job, int n_layers, size_t stride, int h, int w, float* out, hipStream_t stream);

}  // namespace submap
}  // namespace te
