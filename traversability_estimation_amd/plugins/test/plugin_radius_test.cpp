// plugin_radius_test.cpp -- the Step and Roughness plugin adapters with the radii of a fine map: 0.40 m windows and a
// 0.41 m estimation radius on a 0.01 m map are 40 cells, above the 32 the shape kernels hold.  The plugins' context takes
// them (TE_OPT_FILTER_ANY_RADIUS = 1, DeviceMap); update() must return true and match the CPU oracle.  TEST ONLY.
//
//   plugin_radius_test   prints "OK (0 failures)" on success
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <filters/filter_base.h>
#include <grid_map_core/GridMap.hpp>
#include <pluginlib/class_list_macros.h>

#include "te_oracle.h"

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

static int compare(const char* name, const grid_map::Matrix& got, const std::vector<float>& want, bool exact) {
  int bad = 0;
  double mx = 0;
  const size_t n = (size_t)got.rows() * got.cols();
  for (size_t k = 0; k < n; ++k) {
    const float a = got.data()[k], b = want[k];
    if (std::isnan(a) != std::isnan(b)) {
      ++bad;
      continue;
    }
    if (std::isnan(a)) continue;
    const double d = std::fabs((double)a - (double)b);
    if (d > mx) mx = d;
    if (exact ? std::memcmp(&a, &b, 4) != 0 : d > 1e-5) ++bad;
  }
  std::printf("  %-28s mismatches=%d max|d|=%.3g\n", name, bad, mx);
  return bad;
}

int main() {
  const int rows = 160, cols = 140;
  const double res = 0.01;
  grid_map::GridMap map0;
  map0.setGeometry(grid_map::Vec2d{{rows * res, cols * res}}, res, grid_map::Vec2d{{0.35, -0.2}});
  map0.add("elevation");
  grid_map::Matrix& e = map0["elevation"];
  for (int j = 0; j < cols; ++j)
    for (int i = 0; i < rows; ++i) {
      double z = 0.15 * std::sin(0.05 * i) * std::cos(0.04 * j) + 0.002 * ((i * 131 + j * 71) % 17);
      if (i > 60 && i < 90 && j > 50 && j < 75) z += 0.2;  // a box
      e(i, j) = (float)z;
    }
  for (int j = 20; j < 30; ++j)
    for (int i = 100; i < 115; ++i) e(i, j) = std::nanf("");  // an unobserved patch
  const size_t n = (size_t)rows * cols;
  teo_geom g;
  teo_geom_init(&g, rows, cols, res, 0.35, -0.2);
  teo_params p;
  teo_params_default(&p);
  p.normals_radius = 0.335;
  p.rough_radius = 0.412;
  p.step_radius1 = 0.403;
  p.step_radius2 = 0.381;
  std::vector<float> nx(n), ny(n), nz(n), sl(n), st(n), ro(n), tr(n);
  teo_chain(&g, &p, e.data(), sl.data(), st.data(), ro.data(), tr.data(), nx.data(), ny.data(), nz.data());
  // the normals filter runs upstream of the plugins: its layers are inputs here
  map0.add("surface_normal_x");
  map0.add("surface_normal_y");
  map0.add("surface_normal_z");
  std::memcpy(map0["surface_normal_x"].data(), nx.data(), n * 4);
  std::memcpy(map0["surface_normal_y"].data(), ny.data(), n * 4);
  std::memcpy(map0["surface_normal_z"].data(), nz.data(), n * 4);

  auto t = make("filters::StepFilter<grid_map::GridMap>"), r = make("filters::RoughnessFilter<grid_map::GridMap>");
  if (!t || !r) return 1;
  CHECK(t->configure("stepFilter", ParamMap{{"critical_value", p.step_critical}, {"first_window_radius", p.step_radius1},
                                            {"second_window_radius", p.step_radius2}, {"critical_cell_number", p.step_ncrit},
                                            {"map_type", "traversability_step"}}));
  CHECK(r->configure("roughnessFilter", ParamMap{{"critical_value", p.rough_critical}, {"estimation_radius", p.rough_radius},
                                                 {"map_type", "traversability_roughness"}}));
  grid_map::GridMap m1, m2;
  const bool step_ok = t->update(map0, m1);
  CHECK(step_ok);
  const bool rough_ok = step_ok && r->update(m1, m2);
  CHECK(rough_ok);
  if (step_ok && rough_ok) {
    std::printf("plugins at 40 cells on a 0.01 m map:\n");
    CHECK(compare("traversability_step", m2["traversability_step"], st, true) == 0);  // max / min / counts: bit for bit
    CHECK(compare("traversability_roughness", m2["traversability_roughness"], ro, false) == 0);
  }
  if (g_fail == 0) std::printf("OK (0 failures)\n");
  return g_fail == 0 ? 0 : 1;
}
