// The parsers of the two output messages (te_occupancy.h, te_cloud.h: plain host C++) on corrupted inputs:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Itraversability_estimation_amd/csrc
//       tests/cpu/out_msg_check.cpp -o out_msg_check && ./out_msg_check [trials]
// A valid nav_msgs/OccupancyGrid and a valid sensor_msgs/PointCloud2 are written, parsed back and compared; then seeded
// mutations of each (byte flips, extreme and nearby values in 32-bit fields, truncation, spliced garbage) go to the parser in
// exact-size heap buffers.  Every input must be accepted or rejected without a sanitizer report, and an accepted one must
// describe data that lies inside the buffer.  Prints "ok occupancy=<accepted>/<rejected> cloud=<accepted>/<rejected>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "te_cloud.h"
#include "te_occupancy.h"

static int fail(const char* what) {
  printf("FAILED: %s\n", what);
  return 1;
}

static std::vector<uint8_t> mutate(const std::vector<uint8_t>& src, int trial, std::mt19937& rng) {
  std::vector<uint8_t> b(src);
  switch (trial % 4) {
    case 0:
      for (int k = 0; k < 1 + (int)(rng() % 3); ++k) b[rng() % b.size()] = (uint8_t)rng();
      break;
    case 1: {
      const size_t at = rng() % (b.size() - 4);
      uint32_t old;
      memcpy(&old, &b[at], 4);
      const uint32_t vals[] = {0u, 1u, 0x7FFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFF0u, 0x10000u, (uint32_t)b.size(), (uint32_t)(b.size() - at), old + 1, old - 1,
                               (uint32_t)rng()};
      const uint32_t v = vals[rng() % (sizeof(vals) / sizeof(vals[0]))];
      memcpy(&b[at], &v, 4);
      break;
    }
    case 2: b.resize(rng() % b.size()); break;
    default: {
      const size_t at = rng() % b.size(), n = 1 + rng() % 40;
      std::vector<uint8_t> g(n);
      for (auto& x : g) x = (uint8_t)rng();
      b.insert(b.begin() + at, g.begin(), g.end());
    }
  }
  return b;
}

int main(int argc, char** argv) {
  const int trials = argc > 1 ? atoi(argv[1]) : 100000;
  std::string err;

  // ---- a valid occupancy grid, written and read back
  te_occupancy_info oi;
  memset(&oi, 0, sizeof(oi));
  oi.seq = 7;
  oi.stamp_sec = oi.map_load_sec = 12;
  oi.stamp_nsec = oi.map_load_nsec = 34;
  strcpy(oi.frame_id, "odom");
  oi.resolution = 0.05f;
  oi.width = 7;
  oi.height = 5;
  oi.origin[0] = -1.5;
  oi.origin[6] = 1.0;
  size_t need = 0, off = 0;
  if (te::occ::write_skeleton(oi, nullptr, 0, need, off, err)) return fail("the sizing call must not succeed");
  if (need != off + 35) return fail("occupancy size");
  std::vector<uint8_t> omsg(need);
  if (te::occ::write_skeleton(oi, omsg.data(), need - 1, need, off, err)) return fail("a buffer one byte short");
  if (!te::occ::write_skeleton(oi, omsg.data(), need, need, off, err)) return fail("occupancy skeleton");
  for (int k = 0; k < 35; ++k) omsg[off + k] = (uint8_t)(k - 1);
  {
    te_occupancy_info back;
    size_t o2 = 0;
    if (!te::occ::parse(omsg.data(), omsg.size(), back, o2, err)) return fail(err.c_str());
    if (o2 != off || memcmp(&back, &oi, sizeof(oi)) != 0) return fail("occupancy round trip");
  }

  // ---- a valid cloud
  te_cloud_info ci;
  memset(&ci, 0, sizeof(ci));
  ci.seq = 9;
  ci.stamp_sec = 12;
  ci.stamp_nsec = 34;
  strcpy(ci.frame_id, "map");
  ci.width = 6;
  const char* names[4] = {"x", "y", "z", "traversability"};
  if (te::cloud::write_skeleton(ci, te::cloud::Names{4, names}, nullptr, 0, need, off, err)) return fail("the sizing call must not succeed");
  if (need != off + 6 * 16 + 1) return fail("cloud size");
  std::vector<uint8_t> cmsg(need);
  if (!te::cloud::write_skeleton(ci, te::cloud::Names{4, names}, cmsg.data(), need, need, off, err)) return fail("cloud skeleton");
  for (int k = 0; k < 24; ++k) {
    const float v = 0.25f * (float)k;
    memcpy(&cmsg[off + 4 * k], &v, 4);
  }
  {
    te_cloud_info back;
    size_t o2 = 0;
    std::vector<te::cloud::FieldView> fv;
    if (!te::cloud::parse(cmsg.data(), cmsg.size(), back, o2, &fv, err)) return fail(err.c_str());
    if (o2 != off || back.width != 6 || back.height != 1 || back.point_step != 16 || back.row_step != 96 || back.n_fields != 4 || fv.size() != 4)
      return fail("cloud round trip");
    for (int k = 0; k < 4; ++k)
      if (fv[k].name_len != strlen(names[k]) || memcmp(fv[k].name, names[k], fv[k].name_len) != 0 || fv[k].offset != 4u * k || fv[k].datatype != 7 ||
          fv[k].count != 1)
        return fail("cloud fields");
  }

  // ---- mutations
  std::mt19937 rng(1);
  long ok[2] = {0, 0}, bad[2] = {0, 0};
  for (int which = 0; which < 2; ++which) {
    const std::vector<uint8_t>& src = which ? cmsg : omsg;
    for (int trial = 0; trial < trials; ++trial) {
      const std::vector<uint8_t> b = mutate(src, trial, rng);
      uint8_t* heap = (uint8_t*)malloc(b.size() ? b.size() : 1);  // exact size: the sanitizer sees any overrun
      memcpy(heap, b.data(), b.size());
      bool r;
      if (which) {
        te_cloud_info info;
        size_t o = 0;
        std::vector<te::cloud::FieldView> fv;
        r = te::cloud::parse(heap, b.size(), info, o, &fv, err);
        if (r) {
          const unsigned long long data = (unsigned long long)info.row_step * info.height;
          if (o > b.size() || data + 1 > b.size() - o) return fail("cloud data outside the buffer");
          if ((unsigned long long)info.width * info.point_step > info.row_step) return fail("cloud points outside their row");
          for (const auto& f : fv) {
            if ((const uint8_t*)f.name < heap || (const uint8_t*)f.name + f.name_len > heap + b.size()) return fail("field name outside the buffer");
            if ((unsigned long long)f.offset + (unsigned long long)te::cloud::datatype_bytes(f.datatype) * f.count > info.point_step)
              return fail("field outside the point");
          }
          if (strnlen(info.frame_id, TE_MSG_MAX_NAME) >= TE_MSG_MAX_NAME) return fail("cloud frame_id");
        }
      } else {
        te_occupancy_info info;
        size_t o = 0;
        r = te::occ::parse(heap, b.size(), info, o, err);
        if (r) {
          const unsigned long long cells = (unsigned long long)info.width * info.height;
          if (o > b.size() || cells > b.size() - o) return fail("occupancy cells outside the buffer");
          if (strnlen(info.frame_id, TE_MSG_MAX_NAME) >= TE_MSG_MAX_NAME) return fail("occupancy frame_id");
        }
      }
      free(heap);
      (r ? ok : bad)[which]++;
    }
  }
  printf("ok occupancy=%ld/%ld cloud=%ld/%ld\n", ok[0], bad[0], ok[1], bad[1]);
  return 0;
}
