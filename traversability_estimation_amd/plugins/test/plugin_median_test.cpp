// plugin_median_test.cpp -- traversabilityFilters/MedianFillFilter: configure() takes the upstream filter's keys and refuses what
// te_median_fill_params_validate refuses; update() returns the input layer filled on the device, equal bit for bit to the
// contract of include/travgpu.h restated here in a dozen lines (k = 0 and k = 1 openings), and leaves the input layer alone;
// TraversabilityMap::setFillHoles runs the same fill in front of the chain.  TEST ONLY.
//
//   plugin_median_test   prints "OK (0 failures)" on success
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

typedef std::vector<unsigned char> Mask;

static Mask morph(const Mask& m, int rows, int cols, bool erode) {
  Mask out(m.size());
  for (int j = 0; j < cols; ++j)
    for (int i = 0; i < rows; ++i) {
      bool all = true, any = false;
      for (int jj = std::max(j - 1, 0); jj <= std::min(j + 1, cols - 1); ++jj)
        for (int ii = std::max(i - 1, 0); ii <= std::min(i + 1, rows - 1); ++ii) {
          const bool b = m[(size_t)jj * rows + ii] != 0;
          all = all && b;
          any = any || b;
        }
      out[(size_t)j * rows + i] = erode ? all : any;
    }
  return out;
}

// the contract, column-major like grid_map::Matrix; existing values are kept
static std::vector<float> fill(const float* in, int rows, int cols, int r, int k) {
  Mask c((size_t)rows * cols);
  for (size_t n = 0; n < c.size(); ++n) c[n] = std::isfinite(in[n]);
  for (int it = 0; it < k; ++it) c = morph(c, rows, cols, true);
  for (int it = 0; it < k; ++it) c = morph(c, rows, cols, false);
  std::vector<float> out(in, in + c.size());
  for (int j = 0; j < cols; ++j)
    for (int i = 0; i < rows; ++i) {
      if (std::isfinite(in[(size_t)j * rows + i])) continue;
      bool should = false;
      std::vector<float> v;
      for (int jj = std::max(j - r, 0); jj <= std::min(j + r, cols - 1); ++jj)
        for (int ii = std::max(i - r, 0); ii <= std::min(i + r, rows - 1); ++ii) {
          should = should || c[(size_t)jj * rows + ii];
          if (std::isfinite(in[(size_t)jj * rows + ii])) v.push_back(in[(size_t)jj * rows + ii]);
        }
      if (!should || v.empty()) continue;
      std::nth_element(v.begin(), v.begin() + (long)(v.size() / 2), v.end());
      out[(size_t)j * rows + i] = v[v.size() / 2];
    }
  return out;
}

static int differing_bits(const grid_map::Matrix& got, const std::vector<float>& want) {
  int bad = 0;
  for (size_t k = 0; k < want.size(); ++k) bad += std::memcmp(&got.data()[k], &want[k], sizeof(float)) != 0 ? 1 : 0;
  return bad;
}

int main() {
  const char* kFill = "filters::MedianFillFilter<grid_map::GridMap>";
  const int rows = 150, cols = 70;
  const double res = 0.05;
  grid_map::GridMap in;
  in.setGeometry(grid_map::Vec2d{{rows * res, cols * res}}, res, grid_map::Vec2d{{1.25, -0.5}});
  in.add("elevation");
  grid_map::Matrix& e = in["elevation"];
  int holes = 0;
  for (int j = 0; j < cols; ++j)
    for (int i = 0; i < rows; ++i) {
      e(i, j) = (float)(std::floor(40.0 + 30.0 * std::sin(0.11 * i) * std::cos(0.07 * j)) / 255.0);  // k / 255: ties
      if ((i * 131 + j * 71) % 23 == 0 || (i > 100 && j > 40) || (i % 50 == 7 && j % 9 < 4)) {
        e(i, j) = std::nanf("");
        ++holes;
      }
    }
  e(120, 60) = 0.5f;  // an isolated cell inside the unobserved block
  const std::vector<float> input(e.data(), e.data() + (size_t)rows * cols);

  // the keys of the upstream filter; 0.15 / 0.05 truncates to 2 cells
  const ParamMap base{{"input_layer", "elevation"}, {"output_layer", "elevation_inpainted"}, {"fill_hole_radius", 0.15},
                      {"filter_existing_values", 0}, {"existing_value_radius", 0.0}, {"num_erode_dilation_iterations", 0},
                      {"fill_mask_layer", "fill_mask"}, {"debug", 0}};
  for (int k = 0; k <= 1; ++k) {
    auto f = make(kFill);
    ParamMap prm = base;
    prm["num_erode_dilation_iterations"] = k;
    CHECK(f && f->configure("fill", prm));
    grid_map::GridMap out;
    CHECK(f && f->update(in, out));
    CHECK(out.exists("elevation_inpainted") && out.exists("elevation"));
    if (!out.exists("elevation_inpainted")) continue;
    const std::vector<float> want = fill(input.data(), rows, cols, 2, k);
    int filled = 0;
    for (size_t n = 0; n < want.size(); ++n) filled += (!std::isfinite(input[n]) && std::isfinite(want[n])) ? 1 : 0;
    std::printf("MedianFillFilter, k = %d: %d holes, %d filled, %d cells differ from the contract\n", k, holes, filled, differing_bits(out["elevation_inpainted"], want));
    CHECK(filled > 100 && filled < holes);
    CHECK(differing_bits(out["elevation_inpainted"], want) == 0);
    CHECK(differing_bits(out["elevation"], input) == 0);
  }
  // in place: output_layer = input_layer
  {
    auto f = make(kFill);
    ParamMap prm = base;
    prm["output_layer"] = "elevation";
    CHECK(f && f->configure("fill", prm));
    grid_map::GridMap out;
    CHECK(f && f->update(in, out));
    CHECK(differing_bits(out["elevation"], fill(input.data(), rows, cols, 2, 0)) == 0);
  }
  // configure(): the two layers are required, and the ranges are those of te_median_fill_params_validate
  {
    auto f = make(kFill);
    ParamMap prm = base;
    prm.erase("input_layer");
    CHECK(f && !f->configure("fill", prm));
    prm = base;
    prm.erase("output_layer");
    CHECK(f && !f->configure("fill", prm));
    prm = base;
    prm["fill_hole_radius"] = -0.1;
    CHECK(f && !f->configure("fill", prm));
    prm = base;
    prm["num_erode_dilation_iterations"] = -1;
    CHECK(f && !f->configure("fill", prm));
    const ParamMap defaults{{"input_layer", "elevation"}, {"output_layer", "elevation"}};
    CHECK(f && f->configure("fill", defaults));
    grid_map::GridMap none, out;
    none.setGeometry(grid_map::Vec2d{{rows * res, cols * res}}, res, grid_map::Vec2d{{0.0, 0.0}});
    none.add("other");
    CHECK(f && !f->update(none, out));  // the input layer is missing
  }
  // TraversabilityMap::setFillHoles: off by default; on, the chain runs on the filled elevation
  {
    traversability_estimation_gpu::TraversabilityMap map;
    te_median_fill_params p;
    te_median_fill_params_default(&p);
    p.fill_hole_radius = -1.0;
    CHECK(!map.setFillHoles(&p));
    p.fill_hole_radius = 0.15;
    p.num_erode_dilation_iterations = 0;
    CHECK(map.setElevationMap(in));
    CHECK(map.computeTraversability());
    grid_map::GridMap plain = map.getTraversabilityMap();
    CHECK(map.setFillHoles(&p));
    CHECK(map.setElevationMap(in));
    CHECK(map.computeTraversability());
    grid_map::GridMap filled = map.getTraversabilityMap();
    int more = 0, fewer = 0;
    if (plain.exists("traversability") && filled.exists("traversability")) {
      const grid_map::Matrix &a = plain["traversability"], &b = filled["traversability"];
      for (size_t n = 0; n < (size_t)rows * cols; ++n) {
        more += (!std::isfinite(a.data()[n]) && std::isfinite(b.data()[n])) ? 1 : 0;
        fewer += (std::isfinite(a.data()[n]) && !std::isfinite(b.data()[n])) ? 1 : 0;
      }
    }
    std::printf("setFillHoles: %d more cells with a traversability, %d fewer\n", more, fewer);
    CHECK(more > 100 && fewer == 0);
    CHECK(map.setFillHoles(nullptr));
  }
  if (g_fail == 0) std::printf("OK (0 failures)\n");
  return g_fail == 0 ? 0 : 1;
}
