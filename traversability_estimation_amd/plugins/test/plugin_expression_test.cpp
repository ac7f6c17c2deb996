// plugin_expression_test.cpp -- FusedChainFilter with the optional `expression` parameter: the chain's three scores folded
// with a general MathExpressionFilter expression on the device (te_run_expression) equal the oracle chain's scores folded with
// the same expression here, and configure() refuses a text the library refuses.  TEST ONLY.
//
//   plugin_expression_test   prints "OK (0 failures)" on success
#include <cmath>
#include <cstdio>
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

// NaN positions equal, finite cells within tol; returns the mismatches
static int compare(const char* name, const grid_map::Matrix& got, const std::vector<float>& want, double tol) {
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
    if (d > tol) ++bad;
  }
  std::printf("  %-28s mismatches=%d max|d|=%.3g\n", name, bad, mx);
  return bad;
}

int main() {
  const char* kFused = "filters::FusedChainFilter<grid_map::GridMap>";
  const std::string min3 = "cwiseMin(cwiseMin(traversability_slope, traversability_step), traversability_roughness)";
  const int rows = 150, cols = 120;
  const double res = 0.04;
  grid_map::GridMap in;
  in.setGeometry(grid_map::Vec2d{{rows * res, cols * res}}, res, grid_map::Vec2d{{1.25, -0.5}});
  in.add("elevation");
  grid_map::Matrix& e = in["elevation"];
  for (int j = 0; j < cols; ++j)
    for (int i = 0; i < rows; ++i) {
      double z = 0.15 * std::sin(0.11 * i) * std::cos(0.07 * j) + 0.002 * ((i * 131 + j * 71) % 17);
      if (i > 40 && i < 60 && j > 30 && j < 50) z += 0.25;  // a box
      e(i, j) = (float)z;
    }
  e(10, 10) = e(11, 10) = e(100, 90) = std::nanf("");
  const size_t n = (size_t)rows * cols;
  teo_geom g;
  teo_geom_init(&g, rows, cols, res, 1.25, -0.5);
  teo_params p;
  teo_params_default(&p);
  p.normals_radius = 0.09;
  p.rough_radius = 0.13;
  p.step_radius1 = 0.1;
  p.step_radius2 = 0.07;
  std::vector<float> nx(n), ny(n), nz(n), sl(n), st(n), ro(n), tr(n), want(n);
  teo_chain(&g, &p, in["elevation"].data(), sl.data(), st.data(), ro.data(), tr.data(), nx.data(), ny.data(), nz.data());
  int differs = 0;
  for (size_t k = 0; k < n; ++k) {
    const float ab = (st[k] < sl[k]) ? st[k] : sl[k];  // std::min(slope, step)
    want[k] = (ro[k] < ab) ? ro[k] : ab;
    differs += (std::isfinite(want[k]) && std::fabs(want[k] - tr[k]) > 1e-3f) ? 1 : 0;
  }
  CHECK(differs > 100);  // (the expression is not the weighted sum on this map)

  const ParamMap radii{{"normals_radius", p.normals_radius}, {"estimation_radius", p.rough_radius}, {"first_window_radius", p.step_radius1},
                       {"second_window_radius", p.step_radius2}};
  auto f = make(kFused);
  ParamMap with = radii;
  with["expression"] = min3;
  CHECK(f && f->configure("fused", with));
  grid_map::GridMap out;
  CHECK(f && f->update(in, out));
  std::printf("FusedChainFilter, expression = min of the three scores:\n");
  CHECK(out.exists("traversability") && compare("traversability", out["traversability"], want, 1e-5) == 0);
  CHECK(compare("traversability_slope", out["traversability_slope"], sl, 1e-5) == 0);
  // bit for bit the min of the layers the same update returned
  int bits = 0;
  for (size_t k = 0; k < n; ++k) {
    const float a = out["traversability_slope"].data()[k], b = out["traversability_step"].data()[k], c = out["traversability_roughness"].data()[k];
    const float ab = (b < a) ? b : a, m = (c < ab) ? c : ab, got = out["traversability"].data()[k];
    bits += (std::isnan(m) ? !std::isnan(got) : !(m == got)) ? 1 : 0;
  }
  CHECK(bits == 0);
  // without the parameter: the weighted sum, as before
  auto plain = make(kFused);
  CHECK(plain && plain->configure("fused", radii));
  grid_map::GridMap out2;
  CHECK(plain && plain->update(in, out2));
  CHECK(compare("traversability (no expression)", out2["traversability"], tr, 1e-5) == 0);
  // configure() refuses what te_expr_check refuses
  ParamMap bad = radii;
  bad["expression"] = "traversability_slope * traversability_step";  // the matrix product
  CHECK(f && !f->configure("fused", bad));
  bad["expression"] = "traversability_slope +";
  CHECK(f && !f->configure("fused", bad));
  if (g_fail == 0) std::printf("OK (0 failures)\n");
  return g_fail == 0 ? 0 : 1;
}
