// Seeded fuzzer over the compiler of te_expr.h (tests/test_expr_fuzz.py builds it with -fsanitize=address,undefined and runs it
// directly): valid texts, mutated ones, truncated ones, random bytes and nesting 10 000 deep.  What compiles is checked against
// the program's limits and evaluated on a 3-cell input.  Prints "ok compiled=N rejected=M unsupported=K".
#include <cstdio>
#include <cstdlib>
#include <string>

#include "te_expr.h"

using namespace te::expr;

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {  // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}
uint32_t below(uint32_t n) { return rnd() % n; }

const char* const kLayers[] = {"elevation", "traversability_slope", "traversability_step", "traversability_roughness", "traversability",
                               "traversability_footprint", "surface_normal_x", "surface_normal_y", "surface_normal_z", "slope_footprint",
                               "step_footprint", "roughness_footprint", "traversability_x", "traversability_rot", "robot_slope"};
const char* const kUnary[] = {"abs", "sqrt", "square", "exp", "log", "log10", "sin", "cos", "tan", "asin", "acos"};
const char* const kRed[] = {"sum", "mean", "sumOfFinites", "meanOfFinites", "minOfFinites", "maxOfFinites", "numberOfFinites"};
const char* const kOther[] = {"min", "max", "transpose", "trace", "norm", "zeros", "ones", "eye", "nosuchlayer", "x"};
const char* const kNumbers[] = {"0", "1.0", "3.", ".5", "1e3", "2.5E-3", "0.25", "1e400", "00012", "1.0 / 3.0"};
const char* const kBinary[] = {" + ", " - ", " * ", " / ", " .* ", " ./ ", "^", " .^ ", "+", "-", "*", "/"};

std::string gen(int depth, bool in_red) {
  const uint32_t r = below(depth <= 0 ? 3 : 12);
  switch (r) {
    case 0: return kLayers[below(15)];
    case 1: return kNumbers[below(10)];
    case 2: return kLayers[below(4)];
    case 3: return "(" + gen(depth - 1, in_red) + ")";
    case 4: return "-" + gen(depth - 1, in_red);
    case 5: return std::string(kUnary[below(11)]) + "(" + gen(depth - 1, in_red) + ")";
    case 6: return std::string(below(2) ? "cwiseMin(" : "cwiseMax(") + gen(depth - 1, in_red) + ", " + gen(depth - 1, in_red) + ")";
    case 7:
      if (!in_red || below(8) == 0) return std::string(kRed[below(7)]) + "(" + gen(depth - 1, true) + ")";
      return gen(depth - 1, in_red);
    case 8: return below(6) ? gen(depth - 1, in_red) : std::string(kOther[below(10)]) + "(" + gen(depth - 1, in_red) + ")";
    default: return gen(depth - 1, in_red) + kBinary[below(12)] + gen(depth - 1, in_red);
  }
}

struct Stack {
  Vec<1> s[kMaxStack];
  void put(int k, const Vec<1>& v) {
    if (k < 0 || k >= kMaxStack - 1) abort();  // (the top of the stack lives outside: 7 slots at most)
    s[k] = v;
  }
  Vec<1> get(int k) const {
    if (k < 0 || k >= kMaxStack - 1) abort();
    return s[k];
  }
};

struct Source {
  const Program* p;
  int cell;
  Vec<1> layer(int slot) const {
    if (slot < 0 || slot >= p->n_layers) abort();
    static const float k[3] = {0.25f, NAN, -INFINITY};
    return Vec<1>{{k[cell] + (float)p->layer_id[slot]}};
  }
  Vec<1> red(int k) const {
    if (k < 0 || k >= p->n_red) abort();
    return Vec<1>{{1.5f}};
  }
};

long long g_ok = 0, g_bad = 0, g_unsupported = 0;

void feed(const std::string& text) {
  Program p;
  char err[200];
  const int rc = compile(text.c_str(), &p, err, sizeof(err));
  if (rc == kBadParam || rc == kUnsupported) {
    if (!err[0]) abort();  // every refusal carries a message
    ++(rc == kBadParam ? g_bad : g_unsupported);
    return;
  }
  if (rc != kOk) abort();
  ++g_ok;
  if (p.n_code < 1 || p.n_code > kMaxCode || p.n_main < 1 || p.n_main > p.n_code || p.n_layers > kMaxLayers || p.n_red > kMaxRed ||
      p.stack_depth < 1 || p.stack_depth > kMaxStack || p.n_consts > kMaxCode)
    abort();
  for (int k = 0; k < p.n_code; ++k) {
    if (p.op[k] >= kOpCount) abort();
    if (p.op[k] == kPushConst && p.arg[k] >= p.n_consts) abort();
    if (p.op[k] == kPushLayer && p.arg[k] >= p.n_layers) abort();
    if (p.op[k] == kPushRed && (p.arg[k] >= p.n_red || k >= p.n_main)) abort();
  }
  int at = p.n_main;
  for (int r = 0; r < p.n_red; ++r) {
    if (p.red_begin[r] != at || p.red_end[r] <= p.red_begin[r] || p.red_end[r] > p.n_code) abort();
    at = p.red_end[r];
  }
  if (at != p.n_code) abort();
  Stack st;
  volatile float sink = 0.0f;
  for (int cell = 0; cell < 3; ++cell) {
    const Source src{&p, cell};
    for (int r = 0; r < p.n_red; ++r) {
      Partial q = partial_empty();
      partial_add(q, p.red_kind[r], run<1>(p, p.red_begin[r], p.red_end[r], st, src).v[0]);
      sink = partial_result(q, p.red_kind[r], 1);
    }
    sink = run<1>(p, 0, p.n_main, st, src).v[0];
  }
  (void)sink;
}

}  // namespace

int main(int argc, char** argv) {
  const long long n = argc > 1 ? atoll(argv[1]) : 200000;
  for (long long it = 0; it < n; ++it) {
    std::string t = gen(1 + (int)below(6), false);
    switch (below(5)) {
      case 0: break;  // as generated
      case 1:         // mutated: a few bytes replaced, inserted or dropped
        for (int k = 1 + (int)below(3); k > 0 && !t.empty(); --k) {
          const size_t at = below((uint32_t)t.size());
          const char c = "()+-*/.^,= <>'[]:;e1a_\t"[below(23)];
          const uint32_t how = below(3);
          if (how == 0)
            t[at] = c;
          else if (how == 1)
            t.insert(at, 1, c);
          else
            t.erase(at, 1);
        }
        break;
      case 2: t.resize(below((uint32_t)t.size() + 1)); break;  // truncated
      case 3:                                                   // random bytes
        t.assign(below(40), ' ');
        for (char& c : t) c = (char)(1 + below(255));
        break;
      default: t = t + kBinary[below(12)] + gen(3, false); break;
    }
    feed(t);
  }
  // nesting 10 000 deep, every way the grammar recurses: the parser bounds its recursion
  const int deep = 10000;
  feed(std::string(deep, '(') + "elevation" + std::string(deep, ')'));
  feed(std::string(deep, '('));
  feed(std::string(deep, '-') + "elevation");
  {
    std::string t, u, v = "elevation";
    for (int k = 0; k < deep; ++k) t += "abs(", u += "cwiseMin(elevation, ", v += "^-2";
    feed(t + "elevation" + std::string(deep, ')'));
    feed(u + "elevation" + std::string(deep, ')'));
    feed(t);
    feed(v);
  }
  {
    std::string t = "elevation";
    for (int k = 0; k < deep; ++k) t += " + elevation";
    feed(t);  // (flat, but far over 64 instructions)
  }
  printf("ok compiled=%lld rejected=%lld unsupported=%lld\n", g_ok, g_bad, g_unsupported);
  return 0;
}
