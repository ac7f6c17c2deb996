// CPU harness over the window mode of te_expr.h and the window rules of te_window_plan.h: the compiler, the evaluator and the
// folds that te_window_expr.hip instantiates (tests/test_window_expr.py).
//   window_expr_check                                  the built-in checks -> "N checks, F failed checks"
//   window_expr_check compile TEXT LAYER               -> "OK n_instructions n_reductions n_outer stack_depth levels" | "ERR class message"
//   window_expr_check eval TEXT LAYER ROWS COLS W EDGE EMPTY ROUTE IN.bin OUT.bin
//                                                      the same line, and ROWS * COLS float32 (column-major) for a text that
//                                                      compiles; ROUTE 2 walks every cell directly, ROUTE 1 folds stored
//                                                      column partials the way the separable kernel does
// Build: g++ -std=c++17 -O2 -ffp-contract=off.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "te_expr.h"
#include "te_window_plan.h"

using namespace te::expr;
namespace W = te::wexpr;

namespace {

struct Stack {
  Vec<1> s[kMaxStack];
  void put(int k, const Vec<1>& v) { s[k] = v; }
  Vec<1> get(int k) const { return s[k]; }
};
struct Res {
  float r[kMaxRed] = {};
  float get(int k) const { return r[k]; }
};
struct At {
  const float* in;
  int rows, cols;
  float pad;
  float operator()(int row, int col) const {
    if (row < 0 || row >= rows || col < 0 || col >= cols) return pad;
    return in[(size_t)col * rows + row];
  }
};

bool finite_f(float v) { return fabsf(v) < INFINITY; }

// te_window_expr.hip: direct_cell
float direct_cell(const Program& p, int edge, bool empty, int m, At at, int i, int j) {
  Stack st;
  Res res;
  at.pad = NAN;
  const W::Extent e = W::extent(edge, m, at.rows, at.cols, i, j, finite_f(at(i, j)), empty);
  if (!e.visited) return NAN;
  if (edge == W::kMean && e.clipped) at.pad = window_mean_of_finites(at, e.blo, e.bhi, e.bclo, e.bchi);
  for (int level = 0; level < (p.n_outer > 0 ? 2 : 1); ++level)
    for (int r = 0; r < p.n_red; ++r)
      if (p.red_level[r] == level) res.r[r] = window_reduce(p, r, st, res, at, e.rlo, e.rhi, e.clo, e.chi);
  const WindowSource<Res> src{0.0f, &res};
  return run<1>(p, 0, p.n_main, st, src).v[0];
}

// te_window_expr.hip, the separable route: pass A over a whole map (every cell row, every column with the halo), pass B per cell
void separable_map(const Program& p, int edge, bool empty, int m, At at, std::vector<float>& out) {
  const int rows = at.rows, cols = at.cols, tc = cols + 2 * m;
  at.pad = NAN;
  Stack st;
  Res res;
  std::vector<Partial> part((size_t)p.n_red * tc * rows, partial_empty());
  const bool clip = edge == W::kInside || edge == W::kCrop;
  for (int jc = 0; jc < tc; ++jc)
    for (int row = 0; row < rows; ++row) {
      const int col = jc - m;
      if (clip && (col < 0 || col >= cols)) continue;
      const int rlo = clip && row - m < 0 ? 0 : row - m, rhi = clip && row + m > rows - 1 ? rows - 1 : row + m;
      for (int r = 0; r < p.n_red; ++r) part[((size_t)r * tc + jc) * rows + row] = window_column(p, r, st, res, at, col, rlo, rhi);
    }
  for (int j = 0; j < cols; ++j)
    for (int i = 0; i < rows; ++i) {
      const W::Extent e = W::extent(edge, m, rows, cols, i, j, finite_f(at(i, j)), empty);
      float v = NAN;
      if (e.visited) {
        for (int r = 0; r < p.n_red; ++r) {
          Partial acc = partial_empty();
          for (int col = e.clo; col <= e.chi; ++col) partial_merge(acc, part[((size_t)r * tc + (col + m)) * rows + i]);
          res.r[r] = partial_result(acc, p.red_kind[r], (uint64_t)(e.rhi - e.rlo + 1) * (uint64_t)(e.chi - e.clo + 1));
        }
        const WindowSource<Res> src{0.0f, &res};
        v = run<1>(p, 0, p.n_main, st, src).v[0];
      }
      out[(size_t)j * rows + i] = v;
    }
}

// route 1: the separable fold wherever the kernel would take it (no nested reduction; `mean`: cells with a whole window)
void evaluate(const Program& p, int edge, bool empty, int w, int route, const At& at, std::vector<float>& out) {
  const int m = (w - 1) / 2;
  std::vector<float> sep;
  const bool can = route == 1 && p.n_outer == 0 && p.n_red > 0;
  if (can) {
    sep.resize(out.size());
    separable_map(p, edge, empty, m, at, sep);
  }
  for (int j = 0; j < at.cols; ++j)
    for (int i = 0; i < at.rows; ++i) {
      const bool clipped = i - m < 0 || i + m > at.rows - 1 || j - m < 0 || j + m > at.cols - 1;
      const size_t k = (size_t)j * at.rows + i;
      out[k] = can && !(edge == W::kMean && clipped) ? sep[k] : direct_cell(p, edge, empty, m, at, i, j);
    }
}

int g_checks = 0, g_failed = 0;
void check(bool ok, const char* what) {
  ++g_checks;
  if (!ok) {
    ++g_failed;
    printf("FAILED: %s\n", what);
  }
}

int compile_rc(const char* text, int layer, Program* p, std::string* msg = nullptr) {
  char err[256];
  const int rc = compile_window(text, layer, p, err, sizeof(err));
  if (msg) *msg = err;
  return rc;
}

const char* kStdDev = "sqrt(sumOfFinites(square(elevation - meanOfFinites(elevation))) ./ numberOfFinites(elevation))";

void self_checks() {
  Program p;
  std::string msg;
  // the standard deviation: three reductions, the sum an outer one
  check(compile_rc(kStdDev, 0, &p) == kOk, "the standard deviation compiles");
  check(p.n_red == 3 && p.n_outer == 1, "three reductions, one of them outer");
  check(p.red_kind[0] == kSumFinite && p.red_level[0] == 1, "sumOfFinites is the outer one");
  check(p.red_kind[1] == kMeanFinite && p.red_level[1] == 0 && p.red_kind[2] == kCountFinite && p.red_level[2] == 0, "the others are inner");
  check(p.n_layers == 1 && p.layer_id[0] == 0, "one layer");
  bool arg_reads_inner = false;
  for (int k = p.red_begin[0]; k < p.red_end[0]; ++k) arg_reads_inner |= p.op[k] == kPushRed && p.arg[k] == 1;
  check(arg_reads_inner, "the outer argument reads the inner result");
  for (int k = 0; k < p.n_main; ++k) check(p.op[k] != kPushLayer, "the main code pushes no layer");
  check(p.red_end[2] <= p.n_code && p.red_end[1] <= p.n_code && p.red_begin[1] >= p.red_end[0], "the nested argument lies behind the outer ones");
  // compile() is as it was: no nesting, no levels
  char err[256];
  check(compile("sum(meanOfFinites(elevation))", &p, err, sizeof(err)) == kBadParam && strstr(err, "reductions do not nest"), "compile() refuses nesting with its old text");
  check(compile("2 * elevation", &p, err, sizeof(err)) == kOk && p.n_outer == 0 && p.red_level[0] == 0, "compile() leaves a map as the result");
  // the refusals
  check(compile_rc("abs(elevation)", 0, &p, &msg) == kBadParam && msg.find("column 1") != std::string::npos && msg.find("scalar") != std::string::npos, "a map as the result");
  check(compile_rc("elevation", 0, &p) == kBadParam, "the bare layer");
  check(compile_rc("sum(sum(sum(elevation)))", 0, &p, &msg) == kBadParam && msg.find("column 9") != std::string::npos, "depth 3");
  check(compile_rc("meanOfFinites(traversability_slope)", 0, &p, &msg) == kBadParam && msg.find("column 15") != std::string::npos, "a foreign layer");
  check(compile_rc("meanOfFinites(traversability_slope)", 1, &p) == kOk && p.layer_id[0] == 1, "the same text over that layer");
  check(compile_rc("sum(elevation)+sum(elevation)+sum(elevation)+sum(elevation)+sum(elevation)", 0, &p, &msg) == kBadParam && msg.find("more than 4 reductions") != std::string::npos,
        "five reductions");
  check(compile_rc("sum(sum(elevation)+sum(elevation)+sum(elevation)+sum(elevation))", 0, &p, &msg) == kBadParam, "five reductions, nested");
  check(compile_rc("sum(elevation * elevation)", 0, &p) == kUnsupported, "map * map");
  check(compile_rc("sum(elevation .* elevation) ./ 2 ^ 2", 0, &p) == kOk, "scalar .* ./ ^");
  check(compile_rc("2 + 3", 0, &p) == kOk && p.n_red == 0 && p.n_layers == 0, "a constant");
  check(compile_rc("mean(elevation)", 15, &p) == kBadParam && compile_rc("mean(elevation)", -1, &p) == kBadParam, "a bad input layer");
  check(compile_rc(nullptr, 0, &p) == kBadParam && compile_rc("", 0, &p) == kBadParam, "no text");

  // rule 5: the direct fold and the fold over stored column partials give the same bits
  std::mt19937 rng(7);
  const char* texts[] = {"meanOfFinites(elevation)", "sum(elevation)", "mean(elevation)", "sumOfFinites(elevation) - minOfFinites(elevation)",
                         "maxOfFinites(elevation) - minOfFinites(elevation) + numberOfFinites(elevation)", "2 * meanOfFinites(square(elevation)) - minOfFinites(elevation)"};
  const float specials[] = {-0.0f, 0.0f, INFINITY, -INFINITY, NAN, 1.0e12f, -1.0e12f, 1.0f};
  int differ = 0, row_major_differs = 0;
  for (int round = 0; round < 40; ++round) {
    const int rows = 3 + (int)(rng() % 12), cols = 3 + (int)(rng() % 9);
    std::vector<float> in((size_t)rows * cols);
    std::uniform_real_distribution<float> u(-2.0f, 2.0f);
    for (float& v : in) {
      v = u(rng);
      const unsigned k = rng() % 10;
      if (k < 3) v *= 1.0e12f;             // a magnitude ratio of 1e12 inside a window
      if (k == 9 && round % 2) v = specials[rng() % 8];
    }
    const At at{in.data(), rows, cols, NAN};
    std::vector<float> a(in.size()), b(in.size());
    for (const char* text : texts)
      for (int edge = 0; edge < 4; ++edge)
        for (int w : {1, 3, 5, 9}) {
          if (compile_rc(text, 0, &p) != kOk) {
            ++differ;
            continue;
          }
          evaluate(p, edge, round % 3 != 0, w, 2, at, a);
          evaluate(p, edge, round % 3 != 0, w, 1, at, b);
          differ += memcmp(a.data(), b.data(), a.size() * sizeof(float)) != 0;
        }
    // what the rule is for: a row-major double sum of the same window gives other bits somewhere
    for (int i = 2; i + 2 < rows; ++i)
      for (int j = 2; j + 2 < cols; ++j) {
        double by_col = 0.0, by_row = 0.0;
        for (int c = j - 2; c <= j + 2; ++c) {
          double s = 0.0;
          for (int r = i - 2; r <= i + 2; ++r)
            if (finite_f(at(r, c))) s += (double)at(r, c);
          by_col += s;
        }
        for (int r = i - 2; r <= i + 2; ++r)
          for (int c = j - 2; c <= j + 2; ++c)
            if (finite_f(at(r, c))) by_row += (double)at(r, c);
        row_major_differs += memcmp(&by_col, &by_row, sizeof(double)) != 0;
      }
  }
  check(differ == 0, "direct and separable folds: identical bits");
  check(row_major_differs > 0, "a row-major sum differs from the column-order one somewhere");

  // a bounded run over corrupted texts: every one ends in a class and a message, none in a crash or an overrun
  const std::string seeds[] = {kStdDev, "maxOfFinites(elevation) - minOfFinites(elevation)", "2 * meanOfFinites(cwiseMax(elevation, 0.5)) .^ 2"};
  const char alphabet[] = "()+-*/.^,0123456789eE sumean_OfFinitesqrtlvo[]'=<";
  int odd = 0;
  for (int n = 0; n < 20000; ++n) {
    std::string t = seeds[n % 3];
    for (int k = 0, edits = 1 + (int)(rng() % 4); k < edits; ++k) {
      const size_t at_ = rng() % (t.size() + 1);
      switch (rng() % 3) {
        case 0: t.insert(at_, 1, alphabet[rng() % (sizeof(alphabet) - 1)]); break;
        case 1: if (at_ < t.size()) t.erase(at_, 1 + rng() % 3); break;
        default: if (at_ < t.size()) t[at_] = alphabet[rng() % (sizeof(alphabet) - 1)]; break;
      }
    }
    const int rc = compile_rc(t.c_str(), 0, &p, &msg);
    if (rc == kOk) {
      bool sane = p.n_code <= kMaxCode && p.n_red <= kMaxRed && p.n_main <= p.n_code && p.stack_depth <= kMaxStack && p.n_outer <= p.n_red;
      for (int r = 0; r < p.n_red; ++r) sane = sane && p.red_begin[r] <= p.red_end[r] && p.red_end[r] <= p.n_code && p.red_level[r] <= 1;
      for (int k = 0; k < p.n_code; ++k) sane = sane && p.op[k] < kOpCount && (p.op[k] != kPushRed || p.arg[k] < p.n_red) && (p.op[k] != kPushConst || p.arg[k] < p.n_consts);
      // an outer argument reads inner results only, an inner one none
      for (int r = 0; r < p.n_red; ++r)
        for (int k = p.red_begin[r]; k < p.red_end[r]; ++k)
          if (p.op[k] == kPushRed) sane = sane && p.red_level[r] == 1 && p.red_level[p.arg[k]] == 0;
      if (sane) {  // and it runs
        const float cell[9] = {1, 2, 3, 4, NAN, 6, 7, 8, 9};
        const At at{cell, 3, 3, NAN};
        (void)direct_cell(p, W::kCrop, true, 1, at, 1, 1);
      }
      odd += !sane;
    } else {
      odd += !((rc == kBadParam || rc == kUnsupported) && msg.rfind("expression", 0) == 0);
    }
  }
  check(odd == 0, "corrupted texts end in a class and a message");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 1) {
    self_checks();
    printf("%d checks, %d failed checks\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
  }
  const std::string mode = argv[1];
  if (!((mode == "compile" && argc == 4) || (mode == "eval" && argc == 12))) {
    fprintf(stderr, "usage: window_expr_check [compile TEXT LAYER | eval TEXT LAYER ROWS COLS W EDGE EMPTY ROUTE IN.bin OUT.bin]\n");
    return 2;
  }
  Program p;
  char err[256];
  const int rc = compile_window(argv[2], atoi(argv[3]), &p, err, sizeof(err));
  if (rc != kOk) {
    printf("ERR %s %s\n", rc == kBadParam ? "BAD_PARAM" : rc == kUnsupported ? "UNSUPPORTED" : "OTHER", err);
    return 0;
  }
  printf("OK %d %d %d %d", p.n_code, p.n_red, p.n_outer, p.stack_depth);
  for (int r = 0; r < p.n_red; ++r) printf(" %d", p.red_level[r]);
  printf("\n");
  if (mode == "compile") return 0;
  const int rows = atoi(argv[4]), cols = atoi(argv[5]), w = atoi(argv[6]), edge = atoi(argv[7]), empty = atoi(argv[8]), route = atoi(argv[9]);
  if (rows < 1 || cols < 1 || w < 1 || w % 2 == 0 || edge < 0 || edge > 3) {
    fprintf(stderr, "window_expr_check: bad shape, window or edge\n");
    return 2;
  }
  std::vector<float> in((size_t)rows * cols), out(in.size());
  FILE* f = fopen(argv[10], "rb");
  if (!f || fread(in.data(), sizeof(float), in.size(), f) != in.size()) {
    fprintf(stderr, "window_expr_check: cannot read %zu floats from %s\n", in.size(), argv[10]);
    return 2;
  }
  fclose(f);
  evaluate(p, edge, empty != 0, w, route, At{in.data(), rows, cols, NAN}, out);
  f = fopen(argv[11], "wb");
  if (!f || fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) {
    fprintf(stderr, "window_expr_check: cannot write %s\n", argv[11]);
    return 2;
  }
  fclose(f);
  return 0;
}
