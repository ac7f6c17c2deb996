// te_image.h -- sensor_msgs/Image as an input of the device layers (te_image.hip): the wire format's parser (host code) and
// the kernel that converts the raw pixels to float32 and transposes them into a column-major layer.  The C-ABI entry points
// (te_image_parse, te_upload_image, te_upload_image_msg; include/travgpu.h has the semantics) live in te_transfer.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "travgpu.h"

namespace te {
namespace img {

// channels and bytes per channel of an accepted encoding name (not NUL-terminated); false for every other name
bool encoding_layout(const char* name, size_t len, int& channels, int& bytes_per_channel);
// height, width, step, channels, bytes_per_channel of `info` describe an image this library takes
bool check_layout(const te_image_info& info, std::string& err);
// the serialised message -> info and the offset of its step * height pixel bytes
bool parse(const uint8_t* p, size_t n, te_image_info& info, size_t& data_off, std::string& err);

// bytes of the image that are read: every row but the last at the pitch, the last one only as far as its pixels go
inline size_t payload_bytes(const te_image_info& info) {
  return (size_t)(info.height - 1) * (size_t)info.step + (size_t)info.width * info.channels * info.bytes_per_channel;
}
// the kernel reads whole aligned dwords around a pixel: the device copy of the image needs this much behind its payload
constexpr size_t kStagePad = 16;
// thr of addLayerFromImage: (T)(alpha_threshold * maxv), truncated
unsigned alpha_threshold_sample(double alpha_threshold, int bytes_per_channel);

// staged: the image bytes on the device (4-byte aligned, kStagePad readable bytes behind payload_bytes); dst: one map of a
// layer, height x width column-major.  One launch on `stream`.
hipError_t launch_to_layer(const void* staged, const te_image_info& info, float* dst, float lower, float upper, unsigned thr,
                           hipStream_t stream);

}  // namespace img
}  // namespace te
