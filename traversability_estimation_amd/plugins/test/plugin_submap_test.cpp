// plugin_submap_test.cpp -- TraversabilityMap::getTraversabilityMap(position, length, layers, message): the message parses
// (te_msg_parse / te_msg_layer), carries the submap's geometry (te_submap_geometry) and, layer by layer, the cells that
// getTraversabilityMap() returns for the same rectangle.  TEST ONLY.
//
//   plugin_submap_test   prints "OK (0 failures)" on success
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <grid_map_core/GridMap.hpp>

#include "traversability_estimation_gpu/TraversabilityMap.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      std::fprintf(stderr, "CHECK FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                                     \
    }                                                                               \
  } while (0)

// the message against the whole map `out`: geometry, names, cells
static void check_message(const std::vector<uint8_t>& message, const grid_map::GridMap& out, const grid_map::Position& request,
                          const grid_map::Length& length, const std::vector<std::string>& names, const te_msg_info& header) {
  const int rows = out.getSize()(0), cols = out.getSize()(1);
  te_submap_info sub;
  CHECK(te_submap_geometry(rows, cols, out.getResolution(), out.getPosition().x(), out.getPosition().y(), request.x(), request.y(), length.x(),
                           length.y(), &sub) == TE_OK);
  CHECK(sub.ok == 1);
  te_msg_info mi;
  CHECK(te_msg_parse(message.data(), message.size(), &mi) == TE_OK);
  CHECK(mi.rows == sub.rows && mi.cols == sub.cols && mi.start_row == 0 && mi.start_col == 0);
  CHECK(mi.resolution == out.getResolution() && mi.length_x == sub.length_x && mi.length_y == sub.length_y);
  CHECK(mi.pose[0] == sub.pos_x && mi.pose[1] == sub.pos_y && mi.pose[2] == header.pose[2] && mi.pose[6] == header.pose[6]);
  CHECK(mi.seq == header.seq && mi.stamp_sec == header.stamp_sec && mi.stamp_nsec == header.stamp_nsec && std::strcmp(mi.frame_id, header.frame_id) == 0);
  CHECK(mi.n_layers == (int)names.size() && mi.n_basic_layers == 0);
  if (!sub.ok || mi.n_layers != (int)names.size() || mi.rows != sub.rows || mi.cols != sub.cols) return;
  for (int k = 0; k < mi.n_layers; ++k) {
    char name[TE_MSG_MAX_NAME];
    size_t off = 0;
    CHECK(te_msg_layer(message.data(), message.size(), k, name, &off) == TE_OK);
    CHECK(names[k] == name && out.exists(names[k]));
    if (!out.exists(names[k])) continue;
    const grid_map::Matrix& whole = out.get(names[k]);
    int bad = 0;
    for (int j = 0; j < sub.cols; ++j)
      for (int i = 0; i < sub.rows; ++i) {
        const float want = whole(sub.row0 + i, sub.col0 + j);
        bad += std::memcmp(&message[off + ((size_t)j * sub.rows + i) * sizeof(float)], &want, sizeof(float)) != 0;
      }
    CHECK(bad == 0);
  }
}

int main() {
  using traversability_estimation_gpu::TraversabilityMap;
  const int rows = 67, cols = 45;
  const double res = 0.04;
  const grid_map::Position position = {{1.25, -0.5}};
  grid_map::GridMap in;
  in.setGeometry(grid_map::Vec2d{{rows * res, cols * res}}, res, position);
  in.add("elevation");
  grid_map::Matrix& e = in["elevation"];
  for (int i = 0; i < rows; ++i)
    for (int j = 0; j < cols; ++j) {
      double z = 0.5 + 0.35 * std::sin(0.11 * i) * std::cos(0.09 * j) + 0.002 * ((i * 131 + j * 71) % 17);
      if (i > 20 && i < 30 && j > 25 && j < 35) z += 0.1;  // a box
      e(i, j) = (float)z;
      if ((i * 7 + j * 13) % 11 == 0) e(i, j) = std::nanf("");  // holes
    }
  TraversabilityMap map;
  std::vector<uint8_t> message(3, 0x5a);
  const grid_map::Length metre = {{1.0, 1.0}};
  CHECK(!map.getTraversabilityMap(position, metre, {"elevation"}, message) && message.empty());  // nothing there yet
  CHECK(map.setElevationMap(in));
  CHECK(!map.getTraversabilityMap(position, metre, {"traversability"}, message) && !map.error().empty());  // not computed yet
  CHECK(map.computeTraversability());
  const grid_map::GridMap out = map.getTraversabilityMap();

  te_msg_info header = te_msg_info();
  header.seq = 7;
  header.stamp_sec = 1529564943;
  header.stamp_nsec = 122772932;
  std::strcpy(header.frame_id, "odom");
  header.pose[2] = 0.25;
  header.pose[6] = 1.0;
  const std::vector<std::string> scores = {"traversability", "traversability_slope", "traversability_step", "traversability_roughness"};
  // a metre around a point off the centre (odd sizes, a rectangle that starts at an odd row)
  const grid_map::Position off_centre = {{position.x() + 0.43, position.y() - 0.21}};
  CHECK(map.getTraversabilityMap(off_centre, metre, scores, message, &header));
  check_message(message, out, off_centre, metre, scores, header);
  // a request that reaches over two borders is clamped; one layer
  const grid_map::Position corner = {{position.x() + 0.5 * rows * res - 0.1, position.y() - 0.5 * cols * res + 0.05}};
  CHECK(map.getTraversabilityMap(corner, metre, {"elevation"}, message, &header));
  check_message(message, out, corner, metre, {"elevation"}, header);
  // no layer list: every layer of the map, as the service does; no header: an identity orientation
  const grid_map::Length whole = {{10.0, 10.0}};
  CHECK(map.getTraversabilityMap(position, whole, {}, message));
  te_msg_info plain = te_msg_info();
  plain.pose[6] = 1.0;
  check_message(message, out, position, whole, {"elevation", "traversability_slope", "traversability_step", "traversability_roughness", "traversability"},
                plain);
  CHECK(message.size() > (size_t)rows * cols * 5 * sizeof(float));
  // getSubmap refuses a centre outside the map: isSuccess = false, no message, no error
  const grid_map::Position outside = {{position.x() + rows * res, position.y()}};
  message.assign(3, 0x5a);
  CHECK(!map.getTraversabilityMap(outside, metre, scores, message) && message.empty() && map.error().empty());
  // what is not there
  CHECK(!map.getTraversabilityMap(position, metre, {"traversability_footprint"}, message) && !map.error().empty());  // no footprint pass has run
  CHECK(!map.getTraversabilityMap(position, metre, {"elevation", "no_such_layer"}, message) && message.empty());
  const grid_map::Length negative = {{-1.0, 1.0}};
  CHECK(!map.getTraversabilityMap(position, negative, scores, message) && !map.error().empty());
  std::printf("  getTraversabilityMap(position, length, layers, message): %d x %d\n", rows, cols);
  if (g_fail == 0) std::printf("OK (0 failures)\n");
  return g_fail == 0 ? 0 : 1;
}
