// plugin_move_test.cpp -- TraversabilityMap::moveMap(position, info, exposedCells): a map that follows the robot over a larger
// "world" equals, layer by layer, a fresh TraversabilityMap handed the new window at the position moveMap reports -- with
// tie-free radii (results kept: region runs) and with the shipped radii (a tie: the whole chain runs).  TEST ONLY.
//
//   plugin_move_test   prints "OK (0 failures)" on success
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

using traversability_estimation_gpu::TraversabilityMap;

static const int kWorldRows = 120, kWorldCols = 100, kRows = 83, kCols = 61;
static const double kRes = 0.04;

static float world(int i, int j) {
  double z = 0.5 + 0.35 * std::sin(0.11 * i) * std::cos(0.09 * j) + 0.002 * ((i * 131 + j * 71) % 17);
  if (i > 40 && i < 52 && j > 35 && j < 47) z += 0.15;  // a box
  if ((i * 7 + j * 13) % 53 == 0) return std::nanf("");  // holes
  return (float)z;
}

// the window whose first cell is world cell (i0, j0)
static grid_map::GridMap window(int i0, int j0, const grid_map::Position& position) {
  grid_map::GridMap m;
  m.setGeometry(grid_map::Vec2d{{kRows * kRes, kCols * kRes}}, kRes, position);
  m.add("elevation");
  grid_map::Matrix& e = m["elevation"];
  for (int i = 0; i < kRows; ++i)
    for (int j = 0; j < kCols; ++j) e(i, j) = world(i0 + i, j0 + j);
  return m;
}

static int mismatches(const grid_map::Matrix& a, const grid_map::Matrix& b) {
  int bad = 0;
  for (int j = 0; j < kCols; ++j)
    for (int i = 0; i < kRows; ++i) {
      const float x = a(i, j), y = b(i, j);
      if (std::isnan(x) != std::isnan(y) || (!std::isnan(x) && std::fabs(x - y) > 1e-5f)) ++bad;
    }
  return bad;
}

static void one_case(const te_params& params, int want_kept, int kr, int kc) {
  const grid_map::Position position = {{1.25, -0.5}};
  int i0 = 20, j0 = 18;
  TraversabilityMap map, fresh;
  te_move_info info;
  CHECK(!map.moveMap(position, info) && !map.error().empty());  // no elevation map yet
  CHECK(map.setParameters(params) && fresh.setParameters(params));
  CHECK(map.setElevationMap(window(i0, j0, position)));
  CHECK(map.computeTraversability());
  CHECK(map.traversabilityFootprint(params.fp_radius, params.fp_offset));
  // a request of less than half a cell: nothing moves
  const grid_map::Position near = {{position.x() + 0.4 * kRes, position.y()}};
  CHECK(map.moveMap(near, info) && info.n_rects == 0 && info.pos_x == position.x() && info.pos_y == position.y());
  const grid_map::Position request = {{position.x() + kr * kRes + 0.3 * kRes, position.y() + kc * kRes - 0.2 * kRes}};
  CHECK(te_move_geometry(kRows, kCols, kRes, position.x(), position.y(), request.x(), request.y(), &params, &info) == TE_OK);
  CHECK(info.shift_rows == kr && info.shift_cols == kc && info.results_kept == want_kept);
  i0 -= kr;  // old cell i is now cell i + kr: the window starts kr cells earlier in the world
  j0 -= kc;
  std::vector<std::vector<float>> cells(4);
  const float* strips[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int k = 0; k < info.n_rects; ++k) {
    if (!info.rect_exposed[k]) continue;
    const int32_t* r = info.rects[k];
    for (int j = 0; j < r[3]; ++j)
      for (int i = 0; i < r[2]; ++i) cells[k].push_back(world(i0 + r[0] + i, j0 + r[1] + j));
    strips[k] = cells[k].data();
  }
  te_move_info moved;
  CHECK(map.moveMap(request, moved, strips));
  CHECK(std::memcmp(&moved, &info, sizeof(info)) == 0);
  CHECK(map.traversabilityMapInitialized());
  const grid_map::Position held = {{moved.pos_x, moved.pos_y}};
  CHECK(fresh.setElevationMap(window(i0, j0, held)));
  CHECK(fresh.computeTraversability());
  CHECK(fresh.traversabilityFootprint(params.fp_radius, params.fp_offset));
  const grid_map::GridMap got = map.getTraversabilityMap(), want = fresh.getTraversabilityMap();
  CHECK(got.getPosition().x() == held.x() && got.getPosition().y() == held.y());
  for (const char* name : {"elevation", "traversability_slope", "traversability_step", "traversability_roughness", "traversability", "traversability_footprint"}) {
    CHECK(got.exists(name) && want.exists(name));
    if (!got.exists(name) || !want.exists(name)) continue;
    const int bad = mismatches(got.get(name), want.get(name));
    if (bad) std::fprintf(stderr, "  %s: %d cells differ (kept %d, shift %d %d)\n", name, bad, want_kept, kr, kc);
    CHECK(bad == 0);
  }
  std::printf("  moveMap by (%d, %d) cells, results_kept %d: %d rectangles\n", kr, kc, want_kept, moved.n_rects);
}

int main() {
  te_params shipped;
  CHECK(te_params_default(&shipped) == TE_OK);
  te_params tie_free = shipped;
  const double r = 3.0 * kRes * (1.0 + 1e-6);
  tie_free.normals_radius = tie_free.rough_radius = tie_free.step_radius1 = tie_free.step_radius2 = r;
  tie_free.fp_radius = 4.0 * kRes * (1.0 + 1e-6);
  tie_free.fp_offset = 0.0;
  one_case(tie_free, 1, 5, -3);
  one_case(tie_free, 1, 0, 2);
  one_case(shipped, 0, -4, 6);  // step windows of 0.04 m on a 0.04 m map: a one-cell tie
  // hole filling in force: refused, nothing moved
  {
    TraversabilityMap map;
    const grid_map::Position position = {{0.0, 0.0}};
    te_median_fill_params fill;
    te_move_info info;
    CHECK(te_median_fill_params_default(&fill) == TE_OK && map.setFillHoles(&fill));
    CHECK(map.setElevationMap(window(10, 10, position)));
    const grid_map::Position request = {{3 * kRes, 0.0}};
    CHECK(!map.moveMap(request, info) && !map.error().empty() && info.n_rects == 0);
  }
  if (g_fail == 0) std::printf("OK (0 failures)\n");
  return g_fail == 0 ? 0 : 1;
}
