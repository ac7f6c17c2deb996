// te_cloud.h -- sensor_msgs/PointCloud2 on the wire (ROS1 serialisation): writer and validating parser, and the spans of the
// compaction in te_cloud.hip.  Plain host C++ with no HIP in it, so tests/cpu/out_msg_check.cpp builds it alone under the
// sanitizers.  The kernels and the C-ABI entry points (te_download_cloud, te_download_cloud_msg, te_cloud_msg_write,
// te_cloud_parse, te_cloud_field, te_cloud_spans) are in te_cloud.hip; the semantics in include/travgpu.h.
//
// Message layout (little endian):
//   Header{u32 seq; u32 sec; u32 nsec; string frame_id}  u32 height  u32 width
//   PointField[] fields (u32 count; each: string name; u32 offset; u8 datatype; u32 count)
//   u8 is_bigendian  u32 point_step  u32 row_step  u8[] data (u32 length, then the bytes)  u8 is_dense
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "travgpu.h"

static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "fields are copied as they lie: a little-endian host");

namespace te {
namespace cloud {

// The compaction's spans, in cells.  A wavefront ballots 64 cells at a time; a workgroup of the count and scatter kernels
// owns kBlockCells consecutive cells; a workgroup of the scan kernel turns the counts of kScanCounts such workgroups into
// offsets, so its span is kScanCells cells.
constexpr int kWaveCells = 64;
constexpr int kBlockThreads = 256;
constexpr int kBlockIters = 2;
constexpr int kBlockCells = kBlockThreads * kBlockIters;
constexpr int kScanCounts = 256;
constexpr size_t kScanCells = (size_t)kScanCounts * kBlockCells;

constexpr uint8_t kFloat32 = 7;  // sensor_msgs/PointField FLOAT32
// bytes of PointField datatype 1 .. 8 (INT8, UINT8, INT16, UINT16, INT32, UINT32, FLOAT32, FLOAT64)
inline unsigned datatype_bytes(unsigned t) {
  static const unsigned char b[9] = {0, 1, 1, 2, 2, 4, 4, 4, 8};
  return t >= 1 && t <= 8 ? b[t] : 0;
}

struct FieldView {
  const char* name;  // not NUL-terminated, inside the message
  uint32_t name_len, offset, datatype, count;
};

struct Names {
  int n;
  const char* const* v;
};

// A cloud of info.width points of n float32 fields (height 1): everything but the points.  data_off = where the
// width * 4 * n bytes go (the is_dense byte behind them is written here too).  out may be NULL when cap is 0 (sizing).
inline bool write_skeleton(const te_cloud_info& info, Names fields, uint8_t* out, size_t cap, size_t& need, size_t& data_off,
                           std::string& err) {
  if (fields.n <= 0 || fields.n > 4096 || !fields.v) {
    err = "a cloud needs 1 .. 4096 fields";
    return false;
  }
  if (strnlen(info.frame_id, TE_MSG_MAX_NAME) >= TE_MSG_MAX_NAME) {
    err = "frame_id is not NUL-terminated";
    return false;
  }
  const uint32_t step = 4u * (uint32_t)fields.n;
  const unsigned long long bytes = (unsigned long long)info.width * step;
  if (bytes > 0xffffffffull) {
    err = "width * point_step overflows the data length";
    return false;
  }
  size_t at = 12 + 4 + strlen(info.frame_id) + 4 + 4 + 4;
  for (int k = 0; k < fields.n; ++k) {
    if (!fields.v[k]) {
      err = "NULL field name";
      return false;
    }
    at += 4 + strlen(fields.v[k]) + 4 + 1 + 4;
  }
  at += 1 + 4 + 4 + 4;
  data_off = at;
  need = at + (size_t)bytes + 1;
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
  auto put32 = [&put](uint32_t v) { put(&v, 4); };
  auto put8 = [&put](uint8_t v) { put(&v, 1); };
  put32(info.seq);
  put32(info.stamp_sec);
  put32(info.stamp_nsec);
  put32((uint32_t)strlen(info.frame_id));
  put(info.frame_id, strlen(info.frame_id));
  put32(1);  // height
  put32(info.width);
  put32((uint32_t)fields.n);
  for (int k = 0; k < fields.n; ++k) {
    put32((uint32_t)strlen(fields.v[k]));
    put(fields.v[k], strlen(fields.v[k]));
    put32(4u * (uint32_t)k);
    put8(kFloat32);
    put32(1);
  }
  put8(0);  // is_bigendian
  put32(step);
  put32((uint32_t)bytes);  // row_step
  put32((uint32_t)bytes);  // the data's length
  out[data_off + (size_t)bytes] = info.is_dense ? 1 : 0;
  return true;
}

// fields (may be NULL): receives the views of the message's fields
inline bool parse(const uint8_t* p, size_t n, te_cloud_info& info, size_t& data_off, std::vector<FieldView>* fields, std::string& err) {
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
  auto skip = [&](size_t k) {
    if (!ok || k > n - at)
      ok = false;
    else
      at += k;
  };
  memset(&info, 0, sizeof(info));
  uint32_t flen = 0, nf = 0, dlen = 0;
  uint8_t big = 0, dense = 0;
  get(&info.seq, 4);
  get(&info.stamp_sec, 4);
  get(&info.stamp_nsec, 4);
  get(&flen, 4);
  const size_t frame_at = at;
  skip(flen);
  get(&info.height, 4);
  get(&info.width, 4);
  get(&nf, 4);
  // (a field takes at least 13 bytes: a count beyond what is left of the message is a truncation, not a loop)
  if (ok && nf > (n - at) / 13) ok = false;
  std::vector<FieldView> fv;
  bool long_name = false;
  for (uint32_t k = 0; ok && k < nf; ++k) {
    FieldView f = {nullptr, 0, 0, 0, 0};
    uint8_t dt = 0;
    get(&f.name_len, 4);
    f.name = (const char*)p + at;
    skip(f.name_len);
    get(&f.offset, 4);
    get(&dt, 1);
    get(&f.count, 4);
    f.datatype = dt;
    if (ok && f.name_len >= TE_MSG_MAX_NAME) long_name = true;
    if (ok) fv.push_back(f);
  }
  get(&big, 1);
  get(&info.point_step, 4);
  get(&info.row_step, 4);
  get(&dlen, 4);
  if (!ok) {
    err = "cloud message: truncated";
    return false;
  }
  if (flen >= sizeof(info.frame_id)) {
    err = "cloud message: frame_id longer than TE_MSG_MAX_NAME - 1";
    return false;
  }
  if (long_name) {
    err = "cloud message: field name longer than TE_MSG_MAX_NAME - 1";
    return false;
  }
  memcpy(info.frame_id, p + frame_at, flen);
  info.n_fields = nf;
  info.is_bigendian = big;
  for (const FieldView& f : fv) {
    const unsigned b = datatype_bytes(f.datatype);
    char m[160];
    if (!b) {
      snprintf(m, sizeof(m), "cloud message: field datatype %u (1 .. 8)", f.datatype);
      err = m;
      return false;
    }
    if ((unsigned long long)f.offset + (unsigned long long)b * f.count > info.point_step) {
      snprintf(m, sizeof(m), "cloud message: a field of %u x %u bytes at offset %u ends behind point_step %u", f.count, b, f.offset,
               info.point_step);
      err = m;
      return false;
    }
  }
  if ((unsigned long long)info.width * info.point_step > info.row_step) {
    char m[128];
    snprintf(m, sizeof(m), "cloud message: width * point_step = %llu above row_step %u (or it overflows)",
             (unsigned long long)info.width * info.point_step, info.row_step);
    err = m;
    return false;
  }
  if ((unsigned long long)info.row_step * info.height != dlen) {
    char m[128];
    snprintf(m, sizeof(m), "cloud message: %u bytes of data, row_step * height = %llu (or it overflows)", dlen,
             (unsigned long long)info.row_step * info.height);
    err = m;
    return false;
  }
  if (dlen > n - at) {
    err = "cloud message: data truncated";
    return false;
  }
  data_off = at;
  at += dlen;
  get(&dense, 1);
  if (!ok) {
    err = "cloud message: truncated behind the data";
    return false;
  }
  info.is_dense = dense;
  if (fields) fields->swap(fv);
  return true;
}

}  // namespace cloud
}  // namespace te
