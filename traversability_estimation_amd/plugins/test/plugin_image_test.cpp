// plugin_image_test.cpp -- TraversabilityMap::setElevationFromImage: a 64 x 48 mono16 image through the image route and
// computeTraversability() gives, bit for bit, the traversability layer of the same floats sent through setElevationMap.
// TEST ONLY.
//
//   plugin_image_test   prints "OK (0 failures)" on success
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include <grid_map_core/GridMap.hpp>
#include <sensor_msgs/Image.h>

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
  const int rows = 64, cols = 48;
  const double res = 0.04, minHeight = -0.2, maxHeight = 0.6;
  const grid_map::Position position = {{1.25, -0.5}};
  sensor_msgs::Image image;
  image.header.frame_id = "map";
  image.height = rows;
  image.width = cols;
  image.encoding = "mono16";
  image.is_bigendian = 1;
  image.step = cols * 2 + 3;  // an odd pitch
  image.data.assign((size_t)image.step * rows, 0xEE);
  // addLayerFromImage<unsigned short, 1>, restated: the floats the image stands for
  grid_map::GridMap in;
  in.setGeometry(grid_map::Vec2d{{rows * res, cols * res}}, res, position);
  in.add("elevation");
  grid_map::Matrix& e = in["elevation"];
  const float lower = (float)minHeight, upper = (float)maxHeight, maxv = 65535.0f;
  for (int i = 0; i < rows; ++i)
    for (int j = 0; j < cols; ++j) {
      double z = 0.5 + 0.35 * std::sin(0.11 * i) * std::cos(0.09 * j) + 0.002 * ((i * 131 + j * 71) % 17);
      if (i > 20 && i < 30 && j > 25 && j < 35) z += 0.1;  // a box
      const unsigned g = (unsigned)std::lround(z * 65535.0) & 0xffffu;
      image.data[(size_t)i * image.step + 2 * j] = (uint8_t)(g >> 8);
      image.data[(size_t)i * image.step + 2 * j + 1] = (uint8_t)(g & 0xff);
      const float q = (float)g / maxv;
      const float range = upper - lower;
      const float prod = range * q;
      e(i, j) = lower + prod;
    }

  TraversabilityMap fromImage, fromMap;
  CHECK(!fromImage.computeTraversability());  // no elevation yet
  CHECK(fromImage.setElevationFromImage(image, res, position, minHeight, maxHeight));
  CHECK(fromImage.computeTraversability());
  CHECK(fromMap.setElevationMap(in) && fromMap.computeTraversability());
  grid_map::GridMap a = fromImage.getTraversabilityMap(), b = fromMap.getTraversabilityMap();
  CHECK(a.getSize()(0) == rows && a.getSize()(1) == cols && a.getResolution() == res);
  CHECK(a.getPosition().x() == position.x() && a.getPosition().y() == position.y());
  const size_t n = (size_t)rows * cols;
  int n_finite = 0;
  for (const char* layer : {"elevation", "traversability", "traversability_slope", "traversability_step", "traversability_roughness"}) {
    CHECK(a.exists(layer) && b.exists(layer));
    if (!a.exists(layer) || !b.exists(layer)) continue;
    CHECK(std::memcmp(a[layer].data(), b[layer].data(), n * sizeof(float)) == 0);
  }
  if (a.exists("traversability"))
    for (size_t k = 0; k < n; ++k) n_finite += std::isfinite(a["traversability"].data()[k]) ? 1 : 0;
  std::printf("  setElevationFromImage: %d x %d mono16, %d finite traversability cells\n", rows, cols, n_finite);
  CHECK(n_finite > (int)n / 2);
  // what grid_map_ros refuses is refused, and the map stays usable
  sensor_msgs::Image bad = image;
  bad.encoding = "32FC1";
  CHECK(!fromImage.setElevationFromImage(bad, res, position, minHeight, maxHeight) && !fromImage.error().empty());
  bad = image;
  bad.data.pop_back();
  CHECK(!fromImage.setElevationFromImage(bad, res, position, minHeight, maxHeight));
  CHECK(fromImage.traversabilityMapInitialized());
  if (g_fail == 0) std::printf("OK (0 failures)\n");
  return g_fail == 0 ? 0 : 1;
}
