// te_image.hip -- sensor_msgs/Image (ROS1 serialisation) as an input of the device layers: the reference node's image topic
// (TraversabilityEstimation::imageCallback, TraversabilityEstimation.cpp:154-168 -> GridMapRosConverter::initializeFromImage
// and addLayerFromImage).  The parser is host code; the kernel converts the raw pixels and transposes them: the image is
// row-major with a byte pitch, the layer column-major.  Semantics: include/travgpu.h.
//
// Message layout (little endian; sensor_msgs/Image.msg):
//   Header{u32 seq; u32 sec; u32 nsec; string frame_id}  u32 height  u32 width  string encoding  u8 is_bigendian  u32 step
//   u8[] data (u32 length, then the bytes)
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "te_image.h"

static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "samples are assembled for a little-endian host and device");

namespace te {
namespace img {
namespace {

// The integer grey value of a colour pixel, c0 c1 c2 in memory order: OpenCV 4's fixed-point BGR2GRAY as remembered (no
// OpenCV here to pin it against: travgpu.h).  The weights sum to 1 << kGreyShift.
constexpr unsigned kGreyW0 = 3735, kGreyW1 = 19235, kGreyW2 = 9798, kGreyShift = 15;
static_assert(kGreyW0 + kGreyW1 + kGreyW2 == 1u << kGreyShift, "a grey pixel keeps its value");

struct Encoding {
  const char* name;
  int channels, bytes_per_channel;
};
// (grid_map_ros's switch on the cv type of the encoding)
const Encoding kEncodings[] = {{"mono8", 1, 1},  {"8UC1", 1, 1},   {"mono16", 1, 2}, {"16UC1", 1, 2},  {"rgb8", 3, 1},    {"bgr8", 3, 1},
                               {"8UC3", 3, 1},   {"rgba8", 4, 1},  {"bgra8", 4, 1},  {"8UC4", 4, 1},   {"rgb16", 3, 2},   {"bgr16", 3, 2},
                               {"16UC3", 3, 2},  {"rgba16", 4, 2}, {"bgra16", 4, 2}, {"16UC4", 4, 2}};

struct In {
  const uint8_t* p;
  size_t n, at;
  bool ok;
  bool need(size_t k) {
    if (!ok || k > n - at) ok = false;
    return ok;
  }
  uint32_t u32() {
    uint32_t v = 0;
    if (need(4)) {
      memcpy(&v, p + at, 4);
      at += 4;
    }
    return v;
  }
  uint8_t u8() {
    uint8_t v = 0;
    if (need(1)) v = p[at++];
    return v;
  }
  // a string: its bytes stay in the message
  const char* str(uint32_t& len) {
    len = u32();
    const char* s = nullptr;
    if (need(len)) {
      s = (const char*)p + at;
      at += len;
    }
    return s;
  }
};

constexpr int kTile = 64;  // image rows x image columns of one block's tile

// The PIX bytes at byte offset `a` of the image, byte k in bits 8k.. of the result.  `aligned`: every pixel sits on its
// natural boundary (the pitch is a multiple of the pixel, the device copy starts on a boundary), one load of the pixel's
// width.  Otherwise -- an odd pitch, three- and six-byte pixels -- the aligned dwords around the pixel, shifted.
template <int PIX>
__device__ __forceinline__ uint64_t fetch_pixel(const uint8_t* __restrict__ img, size_t a, int aligned) {
  if constexpr (PIX == 1) {
    return img[a];
  } else {
    if constexpr (PIX == 2 || PIX == 4 || PIX == 8) {
      if (aligned) {
        if constexpr (PIX == 2) return *(const uint16_t*)(img + a);
        if constexpr (PIX == 4) return *(const uint32_t*)(img + a);
        if constexpr (PIX == 8) {
          const uint2 v = *(const uint2*)(img + a);
          return ((uint64_t)v.y << 32) | v.x;
        }
      }
    }
    constexpr int K = (PIX + 3) / 4;  // dwords of the result; the pixel lies in K + 1 aligned ones at most
    const uint32_t* w = (const uint32_t*)(img + (a & ~(size_t)3));
    const unsigned sh = (unsigned)(a & 3) * 8;
    uint32_t lo = w[0];
    uint64_t r = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const uint32_t hi = w[k + 1];  // (behind the last pixel: inside the copy's padding, shifted out when sh == 0)
      r |= (uint64_t)(uint32_t)((((uint64_t)hi << 32) | lo) >> sh) << (32 * k);
      lo = hi;
    }
    return r;
  }
}

// addLayerFromImage<T, CH> for one pixel (travgpu.h); the build's -ffp-contract=off keeps the three float operations apart
template <int BPC, int CH>
__device__ __forceinline__ float pixel_value(uint64_t raw, float lower, float range, unsigned thr, int big) {
  unsigned s[CH];
#pragma unroll
  for (int k = 0; k < CH; ++k) {
    if constexpr (BPC == 1) {
      s[k] = (unsigned)(raw >> (8 * k)) & 0xffu;
    } else {
      const unsigned v = (unsigned)(raw >> (16 * k)) & 0xffffu;
      s[k] = big ? ((v & 0xffu) << 8) | (v >> 8) : v;
    }
  }
  if constexpr (CH == 4) {
    if (s[3] < thr) return __uint_as_float(0x7fc00000u);
  }
  unsigned g = s[0];
  if constexpr (CH >= 3) g = (s[0] * kGreyW0 + s[1] * kGreyW1 + s[2] * kGreyW2 + (1u << (kGreyShift - 1))) >> kGreyShift;
  const float maxv = BPC == 1 ? 255.0f : 65535.0f;
  return lower + range * ((float)g / maxv);
}

// One 64 x 64 tile per block and turn: the lanes of a wavefront run along an image row when they read and convert, and
// along a layer column (= down the image rows) when they write.  The tile's rows are padded to 65 floats, so the transposed
// read takes 32 different banks per half wavefront.
template <int BPC, int CH>
__global__ __launch_bounds__(256) void k_image_to_layer(const uint8_t* __restrict__ img, size_t step, size_t height, size_t width,
                                                        float* __restrict__ out, float lower, float range, unsigned thr, int big,
                                                        int aligned, size_t tiles_x, size_t ntiles) {
  constexpr int PIX = BPC * CH;
  __shared__ float tile[kTile][kTile + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const size_t r0 = (t / tiles_x) * kTile, c0 = (t % tiles_x) * kTile;
    if (c0 + lane < width)
      for (int k = wave; k < kTile && r0 + k < height; k += 4)
        tile[k][lane] = pixel_value<BPC, CH>(fetch_pixel<PIX>(img, (r0 + k) * step + (c0 + lane) * PIX, aligned), lower, range, thr, big);
    __syncthreads();
    if (r0 + lane < height)
      for (int k = wave; k < kTile && c0 + k < width; k += 4) out[(c0 + k) * height + r0 + lane] = tile[lane][k];
    __syncthreads();
  }
}

}  // namespace

bool encoding_layout(const char* name, size_t len, int& channels, int& bytes_per_channel) {
  for (const Encoding& e : kEncodings)
    if (strlen(e.name) == len && memcmp(e.name, name, len) == 0) {
      channels = e.channels;
      bytes_per_channel = e.bytes_per_channel;
      return true;
    }
  return false;
}

bool check_layout(const te_image_info& info, std::string& err) {
  char b[160];
  if (info.height <= 0 || info.width <= 0) {
    snprintf(b, sizeof(b), "image of %d x %d pixels", info.height, info.width);
    err = b;
    return false;
  }
  if ((info.channels != 1 && info.channels != 3 && info.channels != 4) || (info.bytes_per_channel != 1 && info.bytes_per_channel != 2)) {
    snprintf(b, sizeof(b), "%d channels of %d bytes (1, 3 or 4 channels of 1 or 2 bytes)", info.channels, info.bytes_per_channel);
    err = b;
    return false;
  }
  const long long row = (long long)info.width * info.channels * info.bytes_per_channel;
  if (row > INT32_MAX) {
    err = "the bytes of an image row overflow";
    return false;
  }
  if (info.step < row) {
    snprintf(b, sizeof(b), "step %d below the %lld bytes of a row", info.step, row);
    err = b;
    return false;
  }
  return true;
}

bool parse(const uint8_t* p, size_t n, te_image_info& info, size_t& data_off, std::string& err) {
  In in = {p, n, 0, true};
  memset(&info, 0, sizeof(info));
  info.seq = in.u32();
  info.stamp_sec = in.u32();
  info.stamp_nsec = in.u32();
  uint32_t frame_len = 0, enc_len = 0;
  const char* frame = in.str(frame_len);
  const uint32_t height = in.u32(), width = in.u32();
  const char* enc = in.str(enc_len);
  const uint8_t big = in.u8();
  const uint32_t step = in.u32(), data_len = in.u32();
  if (!in.ok) {
    err = "image message: truncated";
    return false;
  }
  if (frame_len >= sizeof(info.frame_id)) {
    err = "image message: frame_id longer than TE_MSG_MAX_NAME - 1";
    return false;
  }
  memcpy(info.frame_id, frame, frame_len);
  int channels = 0, bpc = 0;
  if (!encoding_layout(enc, enc_len, channels, bpc)) {
    err = "image message: encoding '" + std::string(enc, enc_len < 32 ? enc_len : 32) + "' (mono8/16, rgb(a)8/16, bgr(a)8/16, 8UCn, 16UCn with n = 1, 3, 4)";
    return false;
  }
  memcpy(info.encoding, enc, enc_len);  // (every accepted name is shorter than the field)
  if (height > (uint32_t)INT32_MAX || width > (uint32_t)INT32_MAX || step > (uint32_t)INT32_MAX) {
    err = "image message: height, width or step overflow";
    return false;
  }
  info.height = (int32_t)height;
  info.width = (int32_t)width;
  info.step = (int32_t)step;
  info.channels = channels;
  info.bytes_per_channel = bpc;
  info.is_bigendian = big;
  if (!check_layout(info, err)) {
    err = "image message: " + err;
    return false;
  }
  if ((unsigned long long)step * height != data_len) {  // (a product beyond 32 bits cannot be a data length)
    char b[128];
    snprintf(b, sizeof(b), "image message: %u bytes of data, step * height = %llu", data_len, (unsigned long long)step * height);
    err = b;
    return false;
  }
  if (!in.need(data_len)) {
    err = "image message: data truncated";
    return false;
  }
  data_off = in.at;
  return true;
}

unsigned alpha_threshold_sample(double alpha_threshold, int bytes_per_channel) {
  const float maxv = bytes_per_channel == 1 ? 255.0f : 65535.0f;
  return (unsigned)(alpha_threshold * maxv);
}

hipError_t launch_to_layer(const void* staged, const te_image_info& info, float* dst, float lower, float upper, unsigned thr,
                           hipStream_t stream) {
  const size_t height = (size_t)info.height, width = (size_t)info.width, step = (size_t)info.step;
  const size_t tiles_x = (width + kTile - 1) / kTile, ntiles = tiles_x * ((height + kTile - 1) / kTile);
  const unsigned blocks = (unsigned)(ntiles < ((size_t)1 << 20) ? ntiles : (size_t)1 << 20);
  const int pix = info.channels * info.bytes_per_channel;
  const int aligned = (pix == 2 || pix == 4 || pix == 8) && step % (size_t)pix == 0;
  const int big = info.is_bigendian != 0;
  const float range = upper - lower;
#define TE_IMAGE_LAUNCH(BPC, CH)                                                                                                      \
  hipLaunchKernelGGL((k_image_to_layer<BPC, CH>), dim3(blocks), dim3(256), 0, stream, (const uint8_t*)staged, step, height, width, dst, \
                     lower, range, thr, big, aligned, tiles_x, ntiles)
  switch (info.bytes_per_channel * 10 + info.channels) {
    case 11: TE_IMAGE_LAUNCH(1, 1); break;
    case 13: TE_IMAGE_LAUNCH(1, 3); break;
    case 14: TE_IMAGE_LAUNCH(1, 4); break;
    case 21: TE_IMAGE_LAUNCH(2, 1); break;
    case 23: TE_IMAGE_LAUNCH(2, 3); break;
    case 24: TE_IMAGE_LAUNCH(2, 4); break;
    default: return hipErrorInvalidValue;
  }
#undef TE_IMAGE_LAUNCH
  return hipGetLastError();
}

}  // namespace img
}  // namespace te
