// plugin_raster_test.cpp -- the SurfaceNormalsFilter and FusedChainFilter adapters with `algorithm: raster`
// (TE_OPT_NORMALS_ALGORITHM on the plugins' context).  The reference of the raster method is the numpy statement of its contract
// (tests/ref_py/raster_normals_ref.py), so this driver computes nothing to compare with: it writes the elevation it used and
// every layer the plugins returned as raw float32 files (column-major, GridMap's own order) into the directory it is given, and
// tests/test_plugins_raster.py holds them to the reference.  An unknown algorithm must make configure() return false.  TEST ONLY.
//
//   plugin_raster_test OUTDIR   prints "OK (0 failures)" on success
#include <cmath>
#include <cstdio>
#include <memory>
#include <string>

#include <filters/filter_base.h>
#include <grid_map_core/GridMap.hpp>
#include <pluginlib/class_list_macros.h>

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

static void dump(const std::string& dir, const std::string& name, grid_map::GridMap& map, const std::string& layer) {
  if (!map.exists(layer)) {
    std::fprintf(stderr, "layer %s missing\n", layer.c_str());
    ++g_fail;
    return;
  }
  const grid_map::Matrix& m = map[layer];
  FILE* f = std::fopen((dir + "/" + name + ".f32").c_str(), "wb");
  const size_t n = (size_t)m.rows() * m.cols();
  if (!f || std::fwrite(m.data(), sizeof(float), n, f) != n) ++g_fail;
  if (f) std::fclose(f);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: plugin_raster_test OUTDIR\n");
    return 2;
  }
  const std::string dir = argv[1];
  const int rows = 67, cols = 45;  // (tests/test_plugins_raster.py states the same geometry and parameters)
  const double res = 0.03;
  grid_map::GridMap map0;
  map0.setGeometry(grid_map::Vec2d{{rows * res, cols * res}}, res, grid_map::Vec2d{{0.4, -1.1}});
  map0.add("elevation");
  grid_map::Matrix& e = map0["elevation"];
  for (int j = 0; j < cols; ++j)
    for (int i = 0; i < rows; ++i) {
      double z = 0.3 * std::sin(0.21 * i) * std::cos(0.17 * j) + 0.02 * i - 0.015 * j + 0.001 * ((i * 131 + j * 71) % 17);
      e(i, j) = (float)z;
      if ((i * 7 + j * 13) % 11 == 0) e(i, j) = std::nanf("");  // scattered holes
    }
  for (int j = 10; j < 18; ++j)
    for (int i = 30; i < 41; ++i) e(i, j) = std::nanf("");  // an unobserved patch
  e(5, 5) = INFINITY;
  e(50, 30) = -INFINITY;
  dump(dir, "elevation", map0, "elevation");

  // SurfaceNormalsFilter, raster, no radius
  auto sn = make("filters::SurfaceNormalsFilter<grid_map::GridMap>");
  if (!sn) return 1;
  CHECK(sn->configure("surfaceNormalsFilter", ParamMap{{"input_layer", "elevation"}, {"output_layers_prefix", "surface_normal_"},
                                                       {"algorithm", "raster"}, {"normal_vector_positive_axis", "z"}}));
  grid_map::GridMap m1;
  const bool sn_ok = sn->update(map0, m1);
  CHECK(sn_ok);
  if (sn_ok)
    for (const char* k : {"surface_normal_x", "surface_normal_y", "surface_normal_z"}) dump(dir, std::string("normals_") + k, m1, k);

  // FusedChainFilter, raster, normals kept
  auto fc = make("filters::FusedChainFilter<grid_map::GridMap>");
  if (!fc) return 1;
  CHECK(fc->configure("fusedChain", ParamMap{{"algorithm", "raster"}, {"estimation_radius", 0.15 * (1.0 + 1e-6)}, {"roughness_critical_value", 0.08},
                                             {"first_window_radius", 0.06 * (1.0 + 1e-6)}, {"second_window_radius", 0.045}, {"keep_surface_normals", 1}}));
  grid_map::GridMap m2;
  const bool fc_ok = fc->update(map0, m2);
  CHECK(fc_ok);
  if (fc_ok)
    for (const char* k : {"surface_normal_x", "surface_normal_y", "surface_normal_z", "traversability_slope", "traversability_step",
                          "traversability_roughness", "traversability"})
      dump(dir, std::string("chain_") + k, m2, k);

  // area again on the same (shared) context: the option goes back with the plugin that asks for it
  auto sa = make("filters::SurfaceNormalsFilter<grid_map::GridMap>");
  if (!sa) return 1;
  CHECK(sa->configure("surfaceNormalsFilter", ParamMap{{"radius", 0.06}, {"algorithm", "area"}}));
  grid_map::GridMap m3;
  const bool sa_ok = sa->update(map0, m3);
  CHECK(sa_ok);
  if (sa_ok) dump(dir, "area_surface_normal_z", m3, "surface_normal_z");

  // an unknown algorithm is refused at configure(); area still needs its radius
  auto bad1 = make("filters::SurfaceNormalsFilter<grid_map::GridMap>"), bad2 = make("filters::FusedChainFilter<grid_map::GridMap>"),
       bad3 = make("filters::SurfaceNormalsFilter<grid_map::GridMap>");
  if (!bad1 || !bad2 || !bad3) return 1;
  CHECK(!bad1->configure("surfaceNormalsFilter", ParamMap{{"radius", 0.05}, {"algorithm", "foo"}}));
  CHECK(!bad2->configure("fusedChain", ParamMap{{"algorithm", "Raster"}}));
  CHECK(!bad3->configure("surfaceNormalsFilter", ParamMap{{"algorithm", "area"}}));

  if (g_fail == 0) std::printf("OK (0 failures)\n");
  return g_fail == 0 ? 0 : 1;
}
