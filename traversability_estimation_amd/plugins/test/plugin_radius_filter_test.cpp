// plugin_radius_filter_test.cpp -- traversabilityFilters/MeanInRadiusFilter and MinInRadiusFilter: configure() takes the upstream
// filters' keys (all three required) and refuses a radius that is negative or not finite; update() returns the input layer
// filtered on the device, equal bit for bit to the contract of include/travgpu.h restated here (the disc decided per centre
// from double positions, row index outer, column index inner, a double sum of the finite values), and leaves the input layer
// alone; TraversabilityMap::setSmoothElevation runs the mean in front of the chain.  TEST ONLY.
//
//   plugin_radius_filter_test   prints "OK (0 failures)" on success
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <filters/filter_base.h>
#include <grid_map_core/GridMap.hpp>
#include <pluginlib/class_list_macros.h>

#include "traversability_estimation_gpu/TraversabilityMap.hpp"

typedef filters::FilterBase<grid_map::GridMap> Filter;
using filters::ParamMap;

static int g_fail = 0;
#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      std::fprintf(stderr, "CHECK FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                                     \
    }                                                                               \
  } while (0)

static std::unique_ptr<Filter> make(const std::string& type) {
  auto it = pluginlib_stub::registry().find(type);
  if (it == pluginlib_stub::registry().end()) {
    std::fprintf(stderr, "class %s not exported\n", type.c_str());
    ++g_fail;
    return nullptr;
  }
  return std::unique_ptr<Filter>(static_cast<Filter*>(it->second()));
}

// the contract, column-major like grid_map::Matrix.  Position of index k along an axis: getPositionFromIndex
static std::vector<float> in_radius(const float* in, int rows, int cols, double res, double px, double py, double radius, bool mean) {
  const double ax = px + (0.5 * (rows * res) - 0.5 * res), ay = py + (0.5 * (cols * res) - 0.5 * res);
  const double r2 = radius * radius;
  const int reach = (int)std::ceil(radius / res) + 1;
  std::vector<float> out((size_t)rows * cols);
  for (int j = 0; j < cols; ++j)
    for (int i = 0; i < rows; ++i) {
      const double cx = ax + res * (double)(-i), cy = ay + res * (double)(-j);
      double sum = 0.0;
      int n = 0;
      float least = std::nanf("");
      for (int ii = std::max(i - reach, 0); ii <= std::min(i + reach, rows - 1); ++ii)
        for (int jj = std::max(j - reach, 0); jj <= std::min(j + reach, cols - 1); ++jj) {
          const double dx = (ax + res * (double)(-ii)) - cx, dy = (ay + res * (double)(-jj)) - cy;
          if (!(dx * dx + dy * dy <= r2)) continue;
          const float v = in[(size_t)jj * rows + ii];
          if (!std::isfinite(v)) continue;
          sum += (double)v;
          ++n;
          if (n == 1 || v < least) least = v;
        }
      out[(size_t)j * rows + i] = n == 0 ? std::nanf("") : (mean ? (float)(sum / n) : least);
    }
  return out;
}

static int differing_bits(const grid_map::Matrix& got, const std::vector<float>& want) {
  int bad = 0;
  for (size_t k = 0; k < want.size(); ++k) bad += std::memcmp(&got.data()[k], &want[k], sizeof(float)) != 0 ? 1 : 0;
  return bad;
}

int main() {
  const char* kMean = "filters::MeanInRadiusFilter<grid_map::GridMap>";
  const char* kMin = "filters::MinInRadiusFilter<grid_map::GridMap>";
  const int rows = 150, cols = 70;
  const double res = 0.05, px = 1.2513, py = -0.5071;  // (no multiple of the resolution: the cells on a circle differ by centre)
  grid_map::GridMap in;
  in.setGeometry(grid_map::Vec2d{{rows * res, cols * res}}, res, grid_map::Vec2d{{px, py}});
  in.add("elevation");
  grid_map::Matrix& e = in["elevation"];
  int holes = 0;
  for (int j = 0; j < cols; ++j)
    for (int i = 0; i < rows; ++i) {
      e(i, j) = (float)(std::floor(40.0 + 30.0 * std::sin(0.11 * i) * std::cos(0.07 * j)) / 255.0 + 0.01 * ((i * 7 + j * 13) % 5));
      if ((i * 131 + j * 71) % 23 == 0 || (i > 100 && j > 40) || (i % 50 == 7 && j % 9 < 4)) {
        e(i, j) = std::nanf("");
        ++holes;
      }
    }
  e(120, 60) = 0.5f;   // an isolated cell inside the unobserved block
  e(20, 20) = INFINITY;  // skipped like NaN
  const std::vector<float> input(e.data(), e.data() + (size_t)rows * cols);

  // radii: 3.5 cells; 3 cells, a whole-cell radius with cells on the circle; 0, the centre cell alone
  for (int op = 0; op < 2; ++op)
    for (double radius : {0.175, 3 * res, 0.0}) {
      auto f = make(op == 0 ? kMean : kMin);
      const ParamMap prm{{"input_layer", "elevation"}, {"output_layer", "elevation_filtered"}, {"radius", radius}};
      CHECK(f && f->configure("radius", prm));
      grid_map::GridMap out;
      CHECK(f && f->update(in, out));
      CHECK(out.exists("elevation_filtered") && out.exists("elevation"));
      if (!out.exists("elevation_filtered")) continue;
      const std::vector<float> want = in_radius(input.data(), rows, cols, res, px, py, radius, op == 0);
      int changed = 0, still = 0;
      for (size_t n = 0; n < want.size(); ++n) {
        changed += std::memcmp(&want[n], &input[n], sizeof(float)) != 0 ? 1 : 0;
        still += std::isfinite(want[n]) ? 0 : 1;
      }
      const int bad = differing_bits(out["elevation_filtered"], want);
      std::printf("%s at %.3f m: %d cells change, %d of %d holes stay, %d cells differ from the contract\n", op == 0 ? "Mean" : "Min", radius, changed, still, holes,
                  bad);
      CHECK(radius == 0.0 ? changed == 1 : (changed > 1000 && still < holes));  // (radius 0: only the infinite cell becomes NaN)
      CHECK(bad == 0);
      CHECK(differing_bits(out["elevation"], input) == 0);
    }
  // in place: output_layer = input_layer
  {
    auto f = make(kMean);
    const ParamMap prm{{"input_layer", "elevation"}, {"output_layer", "elevation"}, {"radius", 0.175}};
    CHECK(f && f->configure("blur", prm));
    grid_map::GridMap out;
    CHECK(f && f->update(in, out));
    CHECK(differing_bits(out["elevation"], in_radius(input.data(), rows, cols, res, px, py, 0.175, true)) == 0);
  }
  // configure(): the three keys are required, the radius is finite and not negative
  for (const char* type : {kMean, kMin}) {
    auto f = make(type);
    const ParamMap base{{"input_layer", "elevation"}, {"output_layer", "lower"}, {"radius", 0.1}};
    for (const char* key : {"input_layer", "output_layer", "radius"}) {
      ParamMap prm = base;
      prm.erase(key);
      CHECK(f && !f->configure("radius", prm));
    }
    ParamMap prm = base;
    prm["radius"] = -0.1;
    CHECK(f && !f->configure("radius", prm));
    prm["radius"] = (double)NAN;
    CHECK(f && !f->configure("radius", prm));
    prm["radius"] = (double)INFINITY;
    CHECK(f && !f->configure("radius", prm));
    CHECK(f && f->configure("radius", base));
    grid_map::GridMap none, out;
    none.setGeometry(grid_map::Vec2d{{rows * res, cols * res}}, res, grid_map::Vec2d{{0.0, 0.0}});
    none.add("other");
    CHECK(f && !f->update(none, out));  // the input layer is missing
  }
  // TraversabilityMap::setSmoothElevation: off by default; on, the chain runs on the smoothed elevation -- the layers are those
  // of a map that was given the plugin's smoothed layer as its elevation
  {
    traversability_estimation_gpu::TraversabilityMap map;
    CHECK(!map.setSmoothElevation(-1.0));
    CHECK(!map.setSmoothElevation((double)NAN));
    CHECK(map.setElevationMap(in));
    CHECK(map.computeTraversability());
    grid_map::GridMap plain = map.getTraversabilityMap();
    CHECK(map.setSmoothElevation(0.175));
    CHECK(map.setElevationMap(in));
    CHECK(map.computeTraversability());
    grid_map::GridMap smoothed = map.getTraversabilityMap();

    auto f = make(kMean);
    const ParamMap prm{{"input_layer", "elevation"}, {"output_layer", "elevation"}, {"radius", 0.175}};
    grid_map::GridMap blurred;
    CHECK(f && f->configure("blur", prm) && f->update(in, blurred));
    CHECK(map.setSmoothElevation(0.0));
    CHECK(map.setElevationMap(blurred));
    CHECK(map.computeTraversability());
    grid_map::GridMap want = map.getTraversabilityMap();
    int differ = 0, moved = 0;
    if (plain.exists("traversability") && smoothed.exists("traversability") && want.exists("traversability")) {
      const grid_map::Matrix &a = plain["traversability"], &b = smoothed["traversability"], &c = want["traversability"];
      for (size_t n = 0; n < (size_t)rows * cols; ++n) {
        differ += std::memcmp(&b.data()[n], &c.data()[n], sizeof(float)) != 0 ? 1 : 0;
        moved += std::memcmp(&a.data()[n], &b.data()[n], sizeof(float)) != 0 ? 1 : 0;
      }
    } else {
      ++g_fail;
    }
    std::printf("setSmoothElevation: %d cells of the traversability move, %d differ from the chain on the smoothed layer\n", moved, differ);
    CHECK(moved > 1000 && differ == 0);
  }
  if (g_fail == 0) std::printf("OK (0 failures)\n");
  return g_fail == 0 ? 0 : 1;
}
