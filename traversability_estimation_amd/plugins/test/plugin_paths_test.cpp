// plugin_paths_test.cpp -- TraversabilityMap::setPathCheckOnDemand(true): a CheckFootprintPath request that mixes two radii
// goes through one on-demand call (te_check_footprint_paths_radius), returns the oracle's results and leaves the layer
// traversabilityFootprint(radius, offset) computed -- and the parameters -- as they were.  TEST ONLY.
//
//   plugin_paths_test   prints "OK (0 failures)" on success
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include <grid_map_core/GridMap.hpp>

#include "te_oracle.h"
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
  const int rows = 150, cols = 120;
  const double res = 0.04, px = 1.25, py = -0.5;
  grid_map::GridMap in;
  in.setGeometry(grid_map::Vec2d{{rows * res, cols * res}}, res, grid_map::Vec2d{{px, py}});
  in.add("elevation");
  grid_map::Matrix& e = in["elevation"];
  for (int j = 0; j < cols; ++j)
    for (int i = 0; i < rows; ++i) {
      double z = 0.12 * std::sin(0.07 * i) * std::cos(0.05 * j) + 0.001 * ((i * 131 + j * 71) % 17);
      if (i > 60 && i < 80 && j > 50 && j < 70) z += 0.3;  // a box
      e(i, j) = (float)z;
    }
  for (int j = 20; j < 30; ++j)
    for (int i = 100; i < 115; ++i) e(i, j) = std::nanf("");  // an unobserved patch
  const size_t n = (size_t)rows * cols;
  teo_geom g;
  teo_geom_init(&g, rows, cols, res, px, py);
  teo_params p;
  teo_params_default(&p);
  p.normals_radius = 0.09;
  p.rough_radius = 0.13;
  p.step_radius1 = 0.1;
  p.step_radius2 = 0.07;
  std::vector<float> sl(n), st(n), ro(n), tr(n);
  const float* elev = e.data();
  teo_chain(&g, &p, elev, sl.data(), st.data(), ro.data(), tr.data(), nullptr, nullptr, nullptr);

  TraversabilityMap tm;
  te_params tp = tm.getParameters();
  tp.normals_radius = p.normals_radius;
  tp.rough_radius = p.rough_radius;
  tp.step_radius1 = p.step_radius1;
  tp.step_radius2 = p.step_radius2;
  CHECK(tm.setParameters(tp));
  CHECK(tm.setElevationMap(in) && tm.computeTraversability());
  CHECK(tm.traversabilityFootprint(0.25, 0.1));  // the user's layer
  grid_map::GridMap before = tm.getTraversabilityMap();
  const te_params params_before = tm.getParameters();
  CHECK(before.exists("traversability_footprint"));

  std::vector<traversability_msgs::FootprintPath> paths;
  unsigned seed = 4711;
  auto rnd = [&]() {
    seed = seed * 1664525u + 1013904223u;
    return (double)(seed >> 8) / (double)(1u << 24);
  };
  for (int k = 0; k < 240; ++k) {
    traversability_msgs::FootprintPath path;
    const int np = 1 + (int)(rnd() * 4.0);
    double x = px + (rnd() - 0.5) * rows * res * 0.95, y = py + (rnd() - 0.5) * cols * res * 0.95;
    for (int m = 0; m < np; ++m) {
      geometry_msgs::Pose pose;
      pose.position.x = x;
      pose.position.y = y;
      pose.orientation.w = 1.0;
      path.poses.poses.push_back(pose);
      x += (rnd() - 0.5) * 0.8;
      y += (rnd() - 0.5) * 0.8;
    }
    path.radius = (k % 2) ? 0.2 : 0.45;
    paths.push_back(path);
  }
  tm.setPathCheckOnDemand(true);
  std::vector<traversability_msgs::TraversabilityResult> results;
  CHECK(tm.checkFootprintPaths(paths, results));
  CHECK(results.size() == paths.size());
  std::vector<float> layer[2] = {std::vector<float>(n), std::vector<float>(n)};
  for (int c = 0; c < 2; ++c) {
    teo_params q = p;
    q.fp_radius = c ? 0.2 : 0.45;
    q.fp_offset = 0.15;
    teo_footprint(&g, &q, elev, sl.data(), st.data(), ro.data(), tr.data(), layer[c].data(), nullptr, nullptr, nullptr);
  }
  int n_safe = 0, n_bad = 0;
  for (size_t k = 0; k < paths.size() && k < results.size(); ++k) {
    const int np = (int)paths[k].poses.poses.size();
    const int off[2] = {0, np};
    unsigned char safe = 0;
    double trav = 0;
    int status = 0;
    std::vector<double> xy;
    for (const auto& pose : paths[k].poses.poses) {
      xy.push_back(pose.position.x);
      xy.push_back(pose.position.y);
    }
    teo_check_circular_paths(&g, layer[k % 2].data(), p.fp_default, 1, off, xy.data(), &safe, &trav, &status);
    const bool both_nan = std::isnan(results[k].traversability) && std::isnan(trav);
    if (results[k].is_safe != safe || (!both_nan && !(std::fabs(results[k].traversability - trav) <= 1e-5)) || results[k].area != 0.0) {
      ++n_bad;
      std::fprintf(stderr, "path %zu: got (%d, %.17g) want (%d, %.17g)\n", k, results[k].is_safe, results[k].traversability, safe, trav);
    }
    n_safe += safe;
  }
  std::printf("  checkFootprintPaths on demand: %zu paths of two radii, %d safe, %d mismatches\n", paths.size(), n_safe, n_bad);
  CHECK(n_bad == 0);
  CHECK(n_safe > 10 && n_safe < (int)paths.size() - 10);
  // the layer of traversabilityFootprint(0.25, 0.1) and the parameters are untouched
  grid_map::GridMap after = tm.getTraversabilityMap();
  CHECK(after.exists("traversability_footprint"));
  if (after.exists("traversability_footprint") && before.exists("traversability_footprint"))
    CHECK(std::memcmp(after["traversability_footprint"].data(), before["traversability_footprint"].data(), n * 4) == 0);
  const te_params params_after = tm.getParameters();
  CHECK(std::memcmp(&params_after, &params_before, sizeof(te_params)) == 0);
  // ... while the default route recomputes it at the paths' radii
  tm.setPathCheckOnDemand(false);
  std::vector<traversability_msgs::TraversabilityResult> dense;
  CHECK(tm.checkFootprintPaths(paths, dense) && dense.size() == results.size());
  int n_diff = 0;
  for (size_t k = 0; k < dense.size() && k < results.size(); ++k)
    if (dense[k].is_safe != results[k].is_safe || std::fabs(dense[k].traversability - results[k].traversability) > 1e-5) ++n_diff;
  CHECK(n_diff == 0);
  grid_map::GridMap later = tm.getTraversabilityMap();
  if (later.exists("traversability_footprint"))
    CHECK(std::memcmp(later["traversability_footprint"].data(), before["traversability_footprint"].data(), n * 4) != 0);
  if (g_fail == 0) std::printf("OK (0 failures)\n");
  return g_fail == 0 ? 0 : 1;
}
