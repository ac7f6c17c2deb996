// plugin_window_expression_test.cpp -- traversabilityFilters/SlidingWindowMathExpressionFilter: configure() takes the upstream
// filter's keys, refuses an entry it cannot honour (a missing key, both or neither window key, an even window, an unknown
// edge handling, an expression the device would refuse); update() returns the expression over the window of every cell,
// computed on the device, equal bit for bit to the contract of include/travgpu.h restated here (columns of the window in
// ascending order, a double sum per column, the column sums added in order), and leaves the input layer alone.  TEST ONLY.
//
//   plugin_window_expression_test   prints "OK (0 failures)" on success
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

// The contract with edge handling `crop` (or `inside`: cells with a clipped window stay NaN), column-major like
// grid_map::Matrix.  kind 0: meanOfFinites(x); 1: sqrt(sumOfFinites(square(x - meanOfFinites(x))) ./ numberOfFinites(x)).
static std::vector<float> window_filter(const float* in, int rows, int cols, int w, bool inside, bool compute_empty, int kind) {
  const int m = (w - 1) / 2;
  std::vector<float> out((size_t)rows * cols, std::nanf(""));
  for (int j = 0; j < cols; ++j)
    for (int i = 0; i < rows; ++i) {
      const bool clipped = i - m < 0 || i + m >= rows || j - m < 0 || j + m >= cols;
      if ((inside && clipped) || (!compute_empty && !std::isfinite(in[(size_t)j * rows + i]))) continue;
      const int r0 = std::max(i - m, 0), r1 = std::min(i + m, rows - 1), c0 = std::max(j - m, 0), c1 = std::min(j + m, cols - 1);
      double sum = 0.0;
      int n = 0;
      for (int c = c0; c <= c1; ++c) {
        double col = 0.0;
        for (int r = r0; r <= r1; ++r) {
          const float v = in[(size_t)c * rows + r];
          if (std::isfinite(v)) col += (double)v, ++n;
        }
        sum += col;
      }
      const float mean = n ? (float)(sum / (double)n) : std::nanf("");
      if (kind == 0) {
        out[(size_t)j * rows + i] = mean;
        continue;
      }
      double dev = 0.0;
      for (int c = c0; c <= c1; ++c) {
        double col = 0.0;
        for (int r = r0; r <= r1; ++r) {
          const float d = in[(size_t)c * rows + r] - mean;  // float32, like every operation of the language
          const float q = d * d;
          if (std::isfinite(q)) col += (double)q;
        }
        dev += col;
      }
      out[(size_t)j * rows + i] = std::sqrt((float)dev / (float)n);
    }
  return out;
}

static int differing_bits(const grid_map::Matrix& got, const std::vector<float>& want) {
  int bad = 0;
  for (size_t k = 0; k < want.size(); ++k) {
    const float a = got.data()[k], b = want[k];
    if (std::isnan(a) && std::isnan(b)) continue;  // (a NaN's payload is not part of the contract)
    bad += std::memcmp(&a, &b, sizeof(float)) != 0 ? 1 : 0;
  }
  return bad;
}

int main() {
  const char* kType = "filters::SlidingWindowMathExpressionFilter<grid_map::GridMap>";
  const char* kStdDev = "sqrt(sumOfFinites(square(elevation - meanOfFinites(elevation))) ./ numberOfFinites(elevation))";
  const int rows = 150, cols = 70;
  const double res = 0.05;
  grid_map::GridMap in;
  in.setGeometry(grid_map::Vec2d{{rows * res, cols * res}}, res, grid_map::Vec2d{{1.25, -0.5}});
  in.add("elevation");
  grid_map::Matrix& e = in["elevation"];
  for (int j = 0; j < cols; ++j)
    for (int i = 0; i < rows; ++i) {
      e(i, j) = (float)(std::floor(40.0 + 30.0 * std::sin(0.11 * i) * std::cos(0.07 * j)) / 255.0 + 0.01 * ((i * 7 + j * 13) % 5));
      if ((i * 131 + j * 71) % 23 == 0 || (i > 100 && j > 40)) e(i, j) = std::nanf("");
    }
  e(20, 20) = INFINITY;  // skipped like NaN
  const std::vector<float> input(e.data(), e.data() + (size_t)rows * cols);

  const ParamMap base{{"input_layer", "elevation"}, {"output_layer", "edges"}, {"expression", kStdDev}, {"window_size", 5},
                      {"compute_empty_cells", 0}, {"edge_handling", "crop"}};
  // the standard deviation of the issue: window 5, crop, compute_empty_cells false; and a box mean through window_length
  for (int kind = 0; kind < 2; ++kind)
    for (int variant = 0; variant < 2; ++variant) {
      auto f = make(kType);
      ParamMap prm = base;
      if (kind == 0) prm["expression"] = "meanOfFinites(elevation)";
      if (variant == 1) {  // window_length 0.15 m at 0.05 m: 3 cells; the defaults: inside, compute_empty_cells true
        prm.erase("window_size");
        prm["window_length"] = 0.15;
        prm.erase("compute_empty_cells");
        prm.erase("edge_handling");
      }
      CHECK(f && f->configure("window", prm));
      grid_map::GridMap out;
      CHECK(f && f->update(in, out));
      CHECK(out.exists("edges") && out.exists("elevation"));
      if (!out.exists("edges")) continue;
      const std::vector<float> want = window_filter(input.data(), rows, cols, variant ? 3 : 5, variant == 1, variant == 1, kind);
      int finite = 0;
      for (float v : want) finite += std::isfinite(v) ? 1 : 0;
      const int bad = differing_bits(out["edges"], want);
      std::printf("%s, %s: %d finite cells, %d cells differ from the contract\n", kind ? "standard deviation" : "box mean",
                  variant ? "window_length 0.15, inside" : "window_size 5, crop", finite, bad);
      CHECK(finite > 5000 && bad == 0);
      CHECK(differing_bits(out["elevation"], input) == 0);
    }
  // another layer name: the expression speaks of the input layer by the name the map gives it
  {
    grid_map::GridMap named = in;
    named.add("height");
    named["height"] = in["elevation"];
    auto f = make(kType);
    ParamMap prm = base;
    prm["input_layer"] = "height";
    prm["expression"] = "maxOfFinites(height) - minOfFinites(height)";
    CHECK(f && f->configure("relief", prm));
    grid_map::GridMap out;
    CHECK(f && f->update(named, out));
    int bad = 0, seen = 0;
    if (out.exists("edges"))
      for (int j = 2; j < cols - 2; ++j)
        for (int i = 2; i < rows - 2; ++i) {
          float lo = INFINITY, hi = -INFINITY;
          for (int c = j - 2; c <= j + 2; ++c)
            for (int r = i - 2; r <= i + 2; ++r) {
              const float v = input[(size_t)c * rows + r];
              if (std::isfinite(v)) lo = std::min(lo, v), hi = std::max(hi, v);
            }
          if (!std::isfinite(input[(size_t)j * rows + i]) || !(lo <= hi)) continue;
          ++seen;
          bad += out["edges"](i, j) == hi - lo ? 0 : 1;
        }
    std::printf("local relief over `height`: %d cells, %d differ\n", seen, bad);
    CHECK(seen > 5000 && bad == 0);
    prm["expression"] = "maxOfFinites(elevation)";  // not the input layer
    CHECK(f && !f->configure("relief", prm));
  }
  // configure(): what cannot be honoured is refused
  {
    auto f = make(kType);
    for (const char* key : {"input_layer", "output_layer", "expression", "window_size"}) {
      ParamMap prm = base;
      prm.erase(key);
      CHECK(f && !f->configure("window", prm));
    }
    ParamMap prm = base;
    prm["window_length"] = 0.25;  // both
    CHECK(f && !f->configure("window", prm));
    for (int bad : {0, 2, 4, -3}) {
      prm = base;
      prm["window_size"] = bad;
      CHECK(f && !f->configure("window", prm));
    }
    for (double bad : {-0.1, (double)NAN, (double)INFINITY}) {
      prm = base;
      prm.erase("window_size");
      prm["window_length"] = bad;
      CHECK(f && !f->configure("window", prm));
    }
    prm = base;
    prm["edge_handling"] = "wrap";
    CHECK(f && !f->configure("window", prm));
    for (const char* text : {"abs(elevation)", "sum(sum(sum(elevation)))", "mean(traversability)", "sum(elevation * elevation)", "mean(elevation"}) {
      prm = base;
      prm["expression"] = text;
      CHECK(f && !f->configure("window", prm));
    }
    CHECK(f && f->configure("window", base));
    grid_map::GridMap none, out;
    none.setGeometry(grid_map::Vec2d{{rows * res, cols * res}}, res, grid_map::Vec2d{{0.0, 0.0}});
    none.add("other");
    CHECK(f && !f->update(none, out));  // the input layer is missing
  }
  if (g_fail == 0) std::printf("OK (0 failures)\n");
  return g_fail == 0 ? 0 : 1;
}
