// te_occupancy.h -- nav_msgs/OccupancyGrid on the wire (ROS1 serialisation): writer and validating parser.  Plain host C++
// with no HIP in it, so tests/cpu/out_msg_check.cpp builds it alone under the sanitizers.  The kernel and the C-ABI entry points
// (te_download_occupancy, te_download_occupancy_msg, te_occupancy_msg_write, te_occupancy_parse) are in te_occupancy.hip; the
// semantics in include/travgpu.h.
//
// Message layout (little endian):
//   Header{u32 seq; u32 sec; u32 nsec; string frame_id}
//   MapMetaData{u32 sec; u32 nsec; f32 resolution; u32 width; u32 height; f64[7] origin}
//   int8[] data (u32 length, then the bytes)
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>

#include "travgpu.h"

static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "fields are copied as they lie: a little-endian host");

namespace te {
namespace occ {

// bytes in front of the cells: header, meta data, the array's length
inline size_t data_offset(const te_occupancy_info& info) { return 12 + 4 + strnlen(info.frame_id, TE_MSG_MAX_NAME) + 8 + 4 + 4 + 4 + 56 + 4; }

// width * height as a data length: false when it does not fit the u32 length field
inline bool cell_count(uint32_t width, uint32_t height, uint32_t& n) {
  const unsigned long long p = (unsigned long long)width * height;
  n = (uint32_t)p;
  return p <= 0xffffffffull;
}

// everything but the cells; data_off = where the width * height bytes go.  out may be NULL when cap is 0 (sizing).
inline bool write_skeleton(const te_occupancy_info& info, uint8_t* out, size_t cap, size_t& need, size_t& data_off, std::string& err) {
  uint32_t n = 0;
  if (!cell_count(info.width, info.height, n)) {
    err = "width * height overflows the data length";
    return false;
  }
  if (strnlen(info.frame_id, TE_MSG_MAX_NAME) >= TE_MSG_MAX_NAME) {
    err = "frame_id is not NUL-terminated";
    return false;
  }
  data_off = data_offset(info);
  need = data_off + n;
  if (cap < need) {
    char b[96];
    snprintf(b, sizeof(b), "buffer of %zu bytes, the message needs %zu", cap, need);
    err = b;
    return false;
  }
  uint8_t* p = out;
  auto put = [&p](const void* v, size_t k) {
    memcpy(p, v, k);
    p += k;
  };
  const uint32_t flen = (uint32_t)strlen(info.frame_id);
  put(&info.seq, 4);
  put(&info.stamp_sec, 4);
  put(&info.stamp_nsec, 4);
  put(&flen, 4);
  put(info.frame_id, flen);
  put(&info.map_load_sec, 4);
  put(&info.map_load_nsec, 4);
  put(&info.resolution, 4);
  put(&info.width, 4);
  put(&info.height, 4);
  put(info.origin, 56);
  put(&n, 4);
  return true;
}

inline bool parse(const uint8_t* p, size_t n, te_occupancy_info& info, size_t& data_off, std::string& err) {
  size_t at = 0;
  bool ok = true;
  auto get = [&](void* v, size_t k) {
    if (!ok || k > n - at) {
      ok = false;
      return;
    }
    memcpy(v, p + at, k);
    at += k;
  };
  memset(&info, 0, sizeof(info));
  uint32_t flen = 0, dlen = 0;
  get(&info.seq, 4);
  get(&info.stamp_sec, 4);
  get(&info.stamp_nsec, 4);
  get(&flen, 4);
  const size_t frame_at = at;
  if (ok && flen > n - at) ok = false;
  if (ok) at += flen;
  get(&info.map_load_sec, 4);
  get(&info.map_load_nsec, 4);
  get(&info.resolution, 4);
  get(&info.width, 4);
  get(&info.height, 4);
  get(info.origin, 56);
  get(&dlen, 4);
  if (!ok) {
    err = "occupancy message: truncated";
    return false;
  }
  if (flen >= sizeof(info.frame_id)) {
    err = "occupancy message: frame_id longer than TE_MSG_MAX_NAME - 1";
    return false;
  }
  memcpy(info.frame_id, p + frame_at, flen);
  uint32_t cells = 0;
  if (!cell_count(info.width, info.height, cells)) {
    err = "occupancy message: width * height overflows";
    return false;
  }
  if (cells != dlen) {
    char b[128];
    snprintf(b, sizeof(b), "occupancy message: %u bytes of data, width * height = %u", dlen, cells);
    err = b;
    return false;
  }
  if (dlen > n - at) {
    err = "occupancy message: data truncated";
    return false;
  }
  data_off = at;
  return true;
}

}  // namespace occ
}  // namespace te
