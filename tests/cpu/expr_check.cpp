// CPU harness over te_expr.h: the compiler and the evaluator the kernels of te_expr.hip instantiate (tests/test_expr.py).
//   expr_check TEXT                           -> "OK n_instructions layer_mask n_reductions stack_depth" | "ERR class message"
//   expr_check TEXT CELLS MAPS IN.bin OUT.bin -> the same line, and for a text that compiles the MAPS * CELLS float32 results
// IN.bin holds the 15 layers in te_layer order, MAPS * CELLS float32 each.  Reductions are taken per map, cell after cell.
// Build: g++ -std=c++17 -O2 -ffp-contract=off.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "te_expr.h"

using namespace te::expr;

namespace {

struct Stack {
  Vec<1> s[kMaxStack];
  void put(int k, const Vec<1>& v) { s[k] = v; }
  Vec<1> get(int k) const { return s[k]; }
};

struct Source {
  const float* const* layers;  // by slot
  size_t cell;                 // flat index
  const float* results;        // of the reductions, for this cell's map
  Vec<1> layer(int slot) const { return Vec<1>{{layers[slot][cell]}}; }
  Vec<1> red(int k) const { return Vec<1>{{results ? results[k] : 0.0f}}; }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2 && argc != 6) {
    fprintf(stderr, "usage: expr_check TEXT [CELLS MAPS IN.bin OUT.bin]\n");
    return 2;
  }
  Program p;
  char err[256];
  const int rc = compile(argv[1], &p, err, sizeof(err));
  if (rc != kOk) {
    printf("ERR %s %s\n", rc == kBadParam ? "BAD_PARAM" : rc == kUnsupported ? "UNSUPPORTED" : "OTHER", err);
    return 0;
  }
  printf("OK %d %u %d %d\n", p.n_code, layer_mask(p), p.n_red, p.stack_depth);
  if (argc == 2) return 0;
  const size_t cells = strtoull(argv[2], nullptr, 10), maps = strtoull(argv[3], nullptr, 10), n = cells * maps;
  std::vector<float> in(15 * n), out(n);
  FILE* f = fopen(argv[4], "rb");
  if (!f || fread(in.data(), sizeof(float), in.size(), f) != in.size()) {
    fprintf(stderr, "expr_check: cannot read %zu floats from %s\n", in.size(), argv[4]);
    return 2;
  }
  fclose(f);
  const float* layers[kMaxLayers] = {};
  for (int k = 0; k < p.n_layers; ++k) layers[k] = in.data() + (size_t)p.layer_id[k] * n;
  Stack st;
  for (size_t m = 0; m < maps; ++m) {
    float red[kMaxRed] = {};
    for (int r = 0; r < p.n_red; ++r) {
      Partial q = partial_empty();
      for (size_t c = 0; c < cells; ++c) {
        const Source src{layers, m * cells + c, nullptr};
        partial_add(q, p.red_kind[r], run<1>(p, p.red_begin[r], p.red_end[r], st, src).v[0]);
      }
      red[r] = partial_result(q, p.red_kind[r], cells);
    }
    for (size_t c = 0; c < cells; ++c) {
      const Source src{layers, m * cells + c, red};
      out[m * cells + c] = run<1>(p, 0, p.n_main, st, src).v[0];
    }
  }
  f = fopen(argv[5], "wb");
  if (!f || fwrite(out.data(), sizeof(float), n, f) != n) {
    fprintf(stderr, "expr_check: cannot write %s\n", argv[5]);
    return 2;
  }
  fclose(f);
  return 0;
}
