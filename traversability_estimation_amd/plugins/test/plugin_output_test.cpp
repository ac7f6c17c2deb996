// plugin_output_test.cpp -- TraversabilityMap::getOccupancyGrid / getPointCloud: the messages equal the conversion of the layers
// getTraversabilityMap() returns, done here on the host with toOccupancyGrid's and toPointCloud's arithmetic restated.
// TEST ONLY.
//
//   plugin_output_test   prints "OK (0 failures)" on success
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
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

int main() {
  using traversability_estimation_gpu::TraversabilityMap;
  const int rows = 67, cols = 45;
  const double res = 0.04;
  const grid_map::Position position = {{1.25, -0.5}};
  grid_map::GridMap in;
  in.setGeometry(grid_map::Vec2d{{rows * res, cols * res}}, res, position);
  in.add("elevation");
  grid_map::Matrix& e = in["elevation"];
  int holes = 0;
  for (int i = 0; i < rows; ++i)
    for (int j = 0; j < cols; ++j) {
      double z = 0.5 + 0.35 * std::sin(0.11 * i) * std::cos(0.09 * j) + 0.002 * ((i * 131 + j * 71) % 17);
      if (i > 20 && i < 30 && j > 25 && j < 35) z += 0.1;  // a box
      e(i, j) = (float)z;
      if ((i * 7 + j * 13) % 11 == 0) {  // holes
        e(i, j) = std::nanf("");
        ++holes;
      }
    }
  TraversabilityMap map;
  nav_msgs::OccupancyGrid grid;
  sensor_msgs::PointCloud2 cloud;
  CHECK(!map.getOccupancyGrid("traversability", 1.0f, 0.0f, grid));  // nothing there yet
  CHECK(!map.getPointCloud({"elevation"}, "elevation", cloud));
  CHECK(map.setElevationMap(in));
  CHECK(!map.getOccupancyGrid("traversability", 1.0f, 0.0f, grid) && !map.error().empty());  // not computed yet
  CHECK(map.computeTraversability());
  grid_map::GridMap out = map.getTraversabilityMap();
  const size_t n = (size_t)rows * cols;

  // ---- the visualization config's four occupancy grids
  int n_unknown = 0;
  grid.header.stamp.sec = 1529564943;
  grid.header.stamp.nsec = 122772932;
  for (const char* layer : {"traversability", "traversability_slope", "traversability_step", "traversability_roughness"}) {
    CHECK(map.getOccupancyGrid(layer, 1.0f, 0.0f, grid));
    CHECK(grid.info.map_load_time.sec == 1529564943 && grid.info.map_load_time.nsec == 122772932);
    CHECK(grid.data.size() == n && grid.info.width == (uint32_t)rows && grid.info.height == (uint32_t)cols);
    CHECK(grid.info.resolution == (float)res);
    CHECK(grid.info.origin.position.x == position.x() - 0.5 * rows * res && grid.info.origin.position.y == position.y() - 0.5 * cols * res);
    CHECK(grid.info.origin.orientation.w == 1.0 && grid.info.origin.orientation.x == 0.0);
    if (!out.exists(layer) || grid.data.size() != n) continue;
    const float* v = out[layer].data();
    int bad = 0;
    for (size_t k = 0; k < n; ++k) {
      const float dataMin = 1.0f, dataMax = 0.0f;
      const float range = dataMax - dataMin;
      const float diff = v[k] - dataMin;
      float value = diff / range;
      int8_t want = -1;
      if (!std::isnan(value)) {
        value = std::min(std::max(0.0f, value), 1.0f);
        const float scaled = value * 100.0f;
        want = (int8_t)(0.0f + scaled);
      } else {
        ++n_unknown;
      }
      bad += grid.data[n - 1 - k] != want;
    }
    CHECK(bad == 0);
  }
  CHECK(n_unknown > 0);
  CHECK(!map.getOccupancyGrid("traversability_footprint", 1.0f, 0.0f, grid));  // no footprint pass has run
  CHECK(!map.getOccupancyGrid("no_such_layer", 1.0f, 0.0f, grid));

  // ---- the elevation cloud, with the traversability as a further field
  CHECK(map.getPointCloud({"traversability", "elevation"}, "elevation", cloud));
  CHECK(cloud.height == 1 && cloud.width == n - holes && cloud.point_step == 16 && cloud.row_step == cloud.width * 16);
  CHECK(cloud.is_bigendian == 0 && cloud.is_dense == 0 && cloud.data.size() == (size_t)cloud.row_step);
  const char* names[4] = {"traversability", "x", "y", "z"};
  CHECK(cloud.fields.size() == 4);
  for (size_t k = 0; k < cloud.fields.size() && k < 4; ++k)
    CHECK(cloud.fields[k].name == names[k] && cloud.fields[k].offset == 4 * k && cloud.fields[k].datatype == 7 && cloud.fields[k].count == 1);
  if (cloud.data.size() == (n - holes) * 16 && out.exists("traversability")) {
    size_t p = 0;
    int bad = 0;
    for (int j = 0; j < cols; ++j)
      for (int i = 0; i < rows; ++i) {
        if (!std::isfinite(e(i, j))) continue;
        // getPosition: centre of cell (i, j)
        const double x = position.x() + (0.5 * (rows * res) - 0.5 * res) + res * (double)(-i);
        const double y = position.y() + (0.5 * (cols * res) - 0.5 * res) + res * (double)(-j);
        const float want[4] = {out["traversability"](i, j), (float)x, (float)y, e(i, j)};
        bad += std::memcmp(&cloud.data[16 * p], want, 16) != 0;
        ++p;
      }
    CHECK(p == n - holes && bad == 0);
  }
  CHECK(!map.getPointCloud({"traversability"}, "elevation", cloud));  // the point layer is not among the layers
  CHECK(!map.getPointCloud({"elevation", "nope"}, "elevation", cloud));
  std::printf("  getOccupancyGrid / getPointCloud: %d x %d, %d holes, %u points\n", rows, cols, holes, cloud.width);
  if (g_fail == 0) std::printf("OK (0 failures)\n");
  return g_fail == 0 ? 0 : 1;
}
