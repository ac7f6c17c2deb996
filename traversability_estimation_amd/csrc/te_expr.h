// te_expr.h -- the expression language of te_run_expression (gridMapFilters/MathExpressionFilter with any expression): a
// compiler from text to a small POD program, and ONE evaluator that the kernels (te_expr.hip) and the CPU check
// (tests/cpu/expr_check.cpp) both instantiate, so the CPU tests pin the code the GPU runs.  The language, its limits and its
// error classes: include/travgpu.h.  EigenLab is not in the reference tree: the semantics are a stated contract restated from
// memory.
//
// The program is postfix code for a stack machine.  `code[0 .. n_main)` is the expression itself; the argument of reduction
// k is the stretch `code[red_begin[k] .. red_end[k])` behind it, evaluated on an empty stack, and the main code reads its
// folded result with kPushRed.  Every value is float32, every operation rounds to float32 (the build's -ffp-contract=off keeps
// them apart).
//
// cwiseMin(a, b) = (b < a) ? b : a and cwiseMax(a, b) = (a < b) ? b : a: std::min / std::max operand order.  NOT symmetric in
// NaN -- a NaN in `a` is returned, a NaN in `b` is dropped.
//
//
// Window mode (compile_window; te_run_window_expression, gridMapFilters/SlidingWindowMathExpressionFilter): the one variable is
// the input layer and denotes the window W around a cell, the result must be a scalar, and reductions nest one level.  A
// reduction whose argument holds reductions is an OUTER one (red_level 1): its argument reads the results of the INNER ones
// (red_level 0) with kPushRed, so the inner ones are folded first.  The folds over W (window_column, window_reduce) are
// defined here once, for both routes of te_window_expr.hip and for the CPU check (tests/cpu/window_expr_check.cpp).
//
// Plain C++17, no HIP types: the parser is host code, the evaluator is marked TE_EXPR_HD.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#if defined(__HIPCC__)
#define TE_EXPR_HD __host__ __device__ __forceinline__
#else
#define TE_EXPR_HD inline
#endif

namespace te {
namespace expr {

constexpr int kMaxCode = 64;    // instructions, reduction arguments included
constexpr int kMaxLayers = 8;   // distinct input layers
constexpr int kMaxStack = 8;    // operand stack, of the main code and of every reduction argument
constexpr int kMaxRed = 4;      // reductions
constexpr int kMaxNesting = 64; // parentheses / prefix signs / calls inside each other: bounds the parser's recursion
// (the values of te_status, include/travgpu.h; te_expr_api.hip asserts that they agree)
constexpr int kOk = 0, kBadParam = -2, kUnsupported = -6;

enum Op : uint8_t {
  kPushLayer = 0,  // arg: slot into layer_id
  kPushConst,      // arg: index into consts
  kPushRed,        // arg: reduction
  kAdd, kSub, kMul, kDiv, kPow, kMin, kMax,  // binary: a = below the top, b = top
  kNeg, kAbs, kSqrt, kSquare, kExp, kLog, kLog10, kSin, kCos, kTan, kAsin, kAcos,
  // Not part of the language, never emitted by the compiler: append_thresholds() puts them behind the main code (ThresholdFilter
  // fused into the expression's pass).  arg: index into consts of the threshold, the replacement behind it.
  kThreshLower,  // top = top < consts[arg] ? consts[arg + 1] : top   (a NaN stays)
  kThreshUpper,  // top = top > consts[arg] ? consts[arg + 1] : top
  kOpCount
};

enum RedKind : uint8_t { kSum = 0, kMean, kSumFinite, kMeanFinite, kMinFinite, kMaxFinite, kCountFinite };

struct Program {
  int32_t n_code;   // all instructions
  int32_t n_main;   // the expression: code[0 .. n_main)
  int32_t n_layers, n_red, n_consts;
  int32_t stack_depth;  // deepest stack of any stretch
  uint8_t op[kMaxCode];
  uint8_t arg[kMaxCode];
  float consts[kMaxCode];
  int32_t layer_id[kMaxLayers];  // te_layer ids
  uint8_t red_kind[kMaxRed];
  uint8_t red_begin[kMaxRed], red_end[kMaxRed];
  uint8_t red_level[kMaxRed];  // window mode: 0 inner (no reduction in its argument), 1 outer; compile() leaves 0
  int32_t n_outer;             // reductions of level 1
};

// ---- the evaluator ---------------------------------------------------------------------------------------------------

// N cells side by side (the kernel: the 4 cells of a 16-byte group; the CPU check: 1)
template <int N>
struct Vec {
  float v[N];
};

TE_EXPR_HD float unary(int op, float x) {
  switch (op) {
    case kNeg: return -x;
    case kAbs: return fabsf(x);
    case kSqrt: return sqrtf(x);
    case kSquare: return x * x;
    case kExp: return expf(x);
    case kLog: return logf(x);
    case kLog10: return log10f(x);
    case kSin: return sinf(x);
    case kCos: return cosf(x);
    case kTan: return tanf(x);
    case kAsin: return asinf(x);
    default: return acosf(x);
  }
}

// ThresholdFilter on one value (te_run_threshold and the two opcodes): the comparison is false for a NaN, which stays
TE_EXPR_HD float threshold_lower(float v, float t, float set_to) { return v < t ? set_to : v; }
TE_EXPR_HD float threshold_upper(float v, float t, float set_to) { return v > t ? set_to : v; }

TE_EXPR_HD float binary(int op, float a, float b) {
  switch (op) {
    case kAdd: return a + b;
    case kSub: return a - b;
    case kMul: return a * b;
    case kDiv: return a / b;
    case kPow: return powf(a, b);
    case kMin: return (b < a) ? b : a;
    default: return (a < b) ? b : a;  // kMax
  }
}

// Runs code[begin .. end) and returns the value it leaves.  The top of the stack is kept in `top`; the values below it live
// in `st` (st.put(slot, value) / st.get(slot)), at most kMaxStack - 1 of them.  `src.layer(slot)` and `src.red(k)` supply
// the operands.  `op` is the same for every cell of a launch: the switch is one branch per instruction, not per cell.
template <int N, class Stack, class Source>
TE_EXPR_HD Vec<N> run(const Program& p, int begin, int end, Stack& st, const Source& src) {
  Vec<N> top;
  for (int k = 0; k < N; ++k) top.v[k] = 0.0f;
  int below = -1;  // slots of `st` in use, minus one; the stretch's first push stores nothing
  bool have = false;
  for (int pc = begin; pc < end; ++pc) {
    const int op = p.op[pc], arg = p.arg[pc];
    if (op <= kPushRed) {
      if (have) st.put(++below, top);
      have = true;
      if (op == kPushLayer) {
        top = src.layer(arg);
      } else if (op == kPushConst) {
        const float c = p.consts[arg];
        for (int k = 0; k < N; ++k) top.v[k] = c;
      } else {
        top = src.red(arg);
      }
    } else if (op < kNeg) {
      const Vec<N> a = st.get(below--);
      switch (op) {
        case kAdd: for (int k = 0; k < N; ++k) top.v[k] = binary(kAdd, a.v[k], top.v[k]); break;
        case kSub: for (int k = 0; k < N; ++k) top.v[k] = binary(kSub, a.v[k], top.v[k]); break;
        case kMul: for (int k = 0; k < N; ++k) top.v[k] = binary(kMul, a.v[k], top.v[k]); break;
        case kDiv: for (int k = 0; k < N; ++k) top.v[k] = binary(kDiv, a.v[k], top.v[k]); break;
        case kPow: for (int k = 0; k < N; ++k) top.v[k] = binary(kPow, a.v[k], top.v[k]); break;
        case kMin: for (int k = 0; k < N; ++k) top.v[k] = binary(kMin, a.v[k], top.v[k]); break;
        default: for (int k = 0; k < N; ++k) top.v[k] = binary(kMax, a.v[k], top.v[k]); break;
      }
    } else {
      switch (op) {
        case kNeg: for (int k = 0; k < N; ++k) top.v[k] = unary(kNeg, top.v[k]); break;
        case kAbs: for (int k = 0; k < N; ++k) top.v[k] = unary(kAbs, top.v[k]); break;
        case kSqrt: for (int k = 0; k < N; ++k) top.v[k] = unary(kSqrt, top.v[k]); break;
        case kSquare: for (int k = 0; k < N; ++k) top.v[k] = unary(kSquare, top.v[k]); break;
        case kExp: for (int k = 0; k < N; ++k) top.v[k] = unary(kExp, top.v[k]); break;
        case kLog: for (int k = 0; k < N; ++k) top.v[k] = unary(kLog, top.v[k]); break;
        case kLog10: for (int k = 0; k < N; ++k) top.v[k] = unary(kLog10, top.v[k]); break;
        case kSin: for (int k = 0; k < N; ++k) top.v[k] = unary(kSin, top.v[k]); break;
        case kCos: for (int k = 0; k < N; ++k) top.v[k] = unary(kCos, top.v[k]); break;
        case kTan: for (int k = 0; k < N; ++k) top.v[k] = unary(kTan, top.v[k]); break;
        case kAsin: for (int k = 0; k < N; ++k) top.v[k] = unary(kAsin, top.v[k]); break;
        case kThreshLower: {
          const float t = p.consts[arg], s = p.consts[arg + 1];
          for (int k = 0; k < N; ++k) top.v[k] = threshold_lower(top.v[k], t, s);
        } break;
        case kThreshUpper: {
          const float t = p.consts[arg], s = p.consts[arg + 1];
          for (int k = 0; k < N; ++k) top.v[k] = threshold_upper(top.v[k], t, s);
        } break;
        default: for (int k = 0; k < N; ++k) top.v[k] = unary(kAcos, top.v[k]); break;
      }
    }
  }
  return top;
}

// A reduction's running state over the cells of one map (or a part of one), and how partial states fold.  `sum` takes every
// value for kSum / kMean and the finite ones otherwise; mn / mx / cnt look at the finite values only.
struct Partial {
  double sum;
  float mn, mx;  // +inf / -inf while no finite value was seen
  uint32_t cnt;  // finite values
  uint32_t _pad;
};

TE_EXPR_HD Partial partial_empty() {
  Partial q;
  q.sum = 0.0;
  q.mn = INFINITY;
  q.mx = -INFINITY;
  q.cnt = 0;
  q._pad = 0;
  return q;
}

TE_EXPR_HD void partial_add(Partial& q, int kind, float x) {
  const bool fin = fabsf(x) < INFINITY;  // (false for NaN)
  if (fin || kind <= kMean) q.sum += (double)x;
  if (fin) {
    q.mn = (x < q.mn) ? x : q.mn;
    q.mx = (q.mx < x) ? x : q.mx;
    q.cnt += 1;
  }
}

TE_EXPR_HD void partial_merge(Partial& q, const Partial& r) {
  q.sum += r.sum;
  q.mn = (r.mn < q.mn) ? r.mn : q.mn;
  q.mx = (q.mx < r.mx) ? r.mx : q.mx;
  q.cnt += r.cnt;
}

// the reduction's float32 result from the state over a whole map of `cells` cells
TE_EXPR_HD float partial_result(const Partial& q, int kind, uint64_t cells) {
  switch (kind) {
    case kSum: return (float)q.sum;
    case kMean: return (float)(q.sum / (double)cells);
    case kSumFinite: return (float)q.sum;
    case kMeanFinite: return q.cnt ? (float)(q.sum / (double)q.cnt) : NAN;
    case kMinFinite: return q.cnt ? q.mn : NAN;
    case kMaxFinite: return q.cnt ? q.mx : NAN;
    default: return (float)q.cnt;
  }
}

// ---- the folds over a window (rule 5 of the window contract, include/travgpu.h) -------------------------------------------
// `at(row, col)` is the value of W at map coordinates (the padding where W reaches beyond the map); `res.get(k)` is the
// result of reduction k for this cell (an outer argument and the main code read them); `st` as in run().

template <class Res>
struct WindowSource {
  float x;
  const Res* res;
  TE_EXPR_HD Vec<1> layer(int) const { return Vec<1>{{x}}; }
  TE_EXPR_HD Vec<1> red(int k) const { return Vec<1>{{res->get(k)}}; }
};

// the Partial of reduction r over one column of W: rows row_lo .. row_hi in ascending order, the sum starting at 0.0
template <class Stack, class Res, class At>
TE_EXPR_HD Partial window_column(const Program& p, int r, Stack& st, const Res& res, const At& at, int col, int row_lo, int row_hi) {
  Partial q = partial_empty();
  const int kind = p.red_kind[r], begin = p.red_begin[r], end = p.red_end[r];
  for (int row = row_lo; row <= row_hi; ++row) {
    const WindowSource<Res> src{at(row, col), &res};
    partial_add(q, kind, run<1>(p, begin, end, st, src).v[0]);
  }
  return q;
}

// reduction r over W = rows [row_lo, row_hi] x columns [col_lo, col_hi]: the column partials folded in ascending column order
template <class Stack, class Res, class At>
TE_EXPR_HD float window_reduce(const Program& p, int r, Stack& st, const Res& res, const At& at, int row_lo, int row_hi, int col_lo, int col_hi) {
  Partial acc = partial_empty();
  for (int col = col_lo; col <= col_hi; ++col) {
    const Partial q = window_column(p, r, st, res, at, col, row_lo, row_hi);
    partial_merge(acc, q);
  }
  return partial_result(acc, p.red_kind[r], (uint64_t)(row_hi - row_lo + 1) * (uint64_t)(col_hi - col_lo + 1));
}

// float32 meanOfFinites of the raw values of a rectangle by the same rule (the padding of edge handling `mean`)
template <class At>
TE_EXPR_HD float window_mean_of_finites(const At& at, int row_lo, int row_hi, int col_lo, int col_hi) {
  Partial acc = partial_empty();
  for (int col = col_lo; col <= col_hi; ++col) {
    Partial q = partial_empty();
    for (int row = row_lo; row <= row_hi; ++row) partial_add(q, kMeanFinite, at(row, col));
    partial_merge(acc, q);
  }
  return partial_result(acc, kMeanFinite, 0);
}

// ---- the compiler (host code) ----------------------------------------------------------------------------------------
struct LayerName {
  const char* name;
  int id;  // te_layer
};
inline const LayerName* layer_names(int* n) {
  static const LayerName k[] = {{"elevation", 0}, {"traversability_slope", 1}, {"traversability_step", 2}, {"traversability_roughness", 3},
                                {"traversability", 4}, {"traversability_footprint", 5}, {"surface_normal_x", 6}, {"surface_normal_y", 7},
                                {"surface_normal_z", 8}, {"slope_footprint", 9}, {"step_footprint", 10}, {"roughness_footprint", 11},
                                {"traversability_x", 12}, {"traversability_rot", 13}, {"robot_slope", 14}};
  *n = (int)(sizeof(k) / sizeof(k[0]));
  return k;
}

class Compiler {
 public:
  // kOk, kBadParam or kUnsupported; on failure `err` (may be NULL) holds the message with the column
  // window_layer >= 0: window mode with that te_layer as the one variable
  // user / n_user: further operand names with their te_layer ids (a context's user layers, te_user_layers.h)
  static int compile(const char* text, Program* out, char* err, size_t err_len, int window_layer = -1, const LayerName* user = nullptr,
                     int n_user = 0) {
    Compiler c(text, err, err_len);
    c.user_ = user;
    c.n_user_ = user ? n_user : 0;
    c.window_ = window_layer >= 0;
    c.win_layer_ = window_layer;
    memset(out, 0, sizeof(*out));
    if (!text) return c.fail(kBadParam, 0, "no expression");
    c.skip();
    if (c.at_end()) return c.fail(kBadParam, c.pos_, "the expression is empty");
    Node n;
    if (!c.parse_expr(0, &n)) return c.rc_;
    c.skip();
    if (!c.at_end()) {
      const char ch = c.s_[c.pos_];
      if (ch == ')') return c.fail(kBadParam, c.pos_, "unbalanced ')'");
      if (ch == '=' || ch == '<' || ch == '>' || ch == '~' || ch == '!' || ch == '&' || ch == '|')
        return c.fail(kUnsupported, c.pos_, "assignment and relational / logical operators are not built");
      if (ch == '\'' || ch == '[' || ch == ']' || ch == ':' || ch == ';')
        return c.fail(kUnsupported, c.pos_, "transpose, matrix literals and ranges are not built");
      if (ch == ',') return c.fail(kBadParam, c.pos_, "unexpected ','");
      return c.fail(kBadParam, c.pos_, "unexpected character");
    }
    if (c.window_ && n.map)
      return c.fail(kBadParam, 0, "the result of a window expression must be a scalar: reduce the window, as in meanOfFinites(...)");
    // main code first, the reduction arguments behind it (window mode: the arguments of nested reductions last)
    Program& p = *out;
    const int n_all = c.n_main_ + c.n_arg_ + c.n_arg2_;
    if (n_all > kMaxCode) return c.fail(kBadParam, c.pos_, "more than 64 instructions");
    for (int k = 0; k < n_all; ++k) {
      const Ins& i = k < c.n_main_ ? c.main_[k] : k < c.n_main_ + c.n_arg_ ? c.argc_[k - c.n_main_] : c.arg2_[k - c.n_main_ - c.n_arg_];
      p.op[k] = i.op;
      p.arg[k] = i.arg;
      if (i.op == kPushConst) {
        int j = 0;
        while (j < p.n_consts && memcmp(&p.consts[j], &i.value, sizeof(float)) != 0) ++j;
        if (j == p.n_consts) p.consts[p.n_consts++] = i.value;
        p.arg[k] = (uint8_t)j;
      }
    }
    p.n_main = c.n_main_;
    p.n_code = n_all;
    p.n_layers = c.n_layers_;
    p.n_red = c.n_red_;
    p.stack_depth = c.max_depth_;
    for (int k = 0; k < kMaxLayers; ++k) p.layer_id[k] = k < c.n_layers_ ? c.layer_id_[k] : -1;
    for (int k = 0; k < c.n_red_; ++k) {
      p.red_kind[k] = c.red_kind_[k];
      const int base = c.n_main_ + (c.red_stream_[k] == 2 ? c.n_arg_ : 0);
      p.red_begin[k] = (uint8_t)(base + c.red_begin_[k]);
      p.red_end[k] = (uint8_t)(base + c.red_end_[k]);
      p.red_level[k] = c.red_level_[k];
      p.n_outer += c.red_level_[k];
    }
    return kOk;
  }

  // a name the language gives a meaning: a function, a reduction, or an EigenLab function it refuses by name
  static bool is_function_name(const char* s, size_t n) { return find_fn(s, n) != nullptr; }

 private:
  struct Ins {
    uint8_t op, arg;
    float value;  // of a kPushConst: the table of constants is built from the code that is left at the end
  };
  struct Node {
    bool map = false;    // a map; otherwise a scalar (1 x 1)
    bool konst = false;  // a scalar known now: its code is the one kPushConst at the end of the stream
    float value = 0.0f;
  };

  Compiler(const char* text, char* err, size_t err_len) : s_(text ? text : ""), len_(strlen(s_)), err_(err), err_len_(err_len) {
    if (err_ && err_len_) err_[0] = 0;
  }

  const char* s_;
  size_t len_;
  size_t pos_ = 0;
  char* err_;
  size_t err_len_;
  int rc_ = kOk;
  Ins main_[kMaxCode + 1], argc_[kMaxCode + 1], arg2_[kMaxCode + 1];
  int n_main_ = 0, n_arg_ = 0, n_arg2_ = 0;
  const LayerName* user_ = nullptr;  // operand names beside the reference's
  int n_user_ = 0;
  bool window_ = false;  // window mode
  int win_layer_ = -1;
  int red_depth_ = 0;  // reductions around the code being emitted: 0 the main code, 1 a reduction's argument, 2 a nested one's
  int depth_ = 0, max_depth_ = 0;
  int layer_id_[kMaxLayers] = {};
  int n_layers_ = 0;
  int n_red_ = 0;
  uint8_t red_kind_[kMaxRed] = {};
  int red_begin_[kMaxRed] = {}, red_end_[kMaxRed] = {};
  int red_stream_[kMaxRed] = {};       // 1: argc_, 2: arg2_
  uint8_t red_level_[kMaxRed] = {};

  bool at_end() const { return pos_ >= len_; }
  void skip() {
    while (pos_ < len_ && (s_[pos_] == ' ' || s_[pos_] == '\t' || s_[pos_] == '\n' || s_[pos_] == '\r')) ++pos_;
  }
  int fail(int rc, size_t col, const char* what) {
    rc_ = rc;
    if (err_ && err_len_) snprintf(err_, err_len_, "expression, column %zu: %s", col + 1, what);
    return rc;
  }
  bool failb(int rc, size_t col, const char* what) {
    fail(rc, col, what);
    return false;
  }

  Ins* stream() { return red_depth_ == 0 ? main_ : red_depth_ == 1 ? argc_ : arg2_; }
  int& count() { return red_depth_ == 0 ? n_main_ : red_depth_ == 1 ? n_arg_ : n_arg2_; }

  // pushes grow the stack by one, binary operators shrink it by one
  bool emit(uint8_t op, uint8_t arg, size_t col) {
    if (n_main_ + n_arg_ + n_arg2_ >= kMaxCode) return failb(kBadParam, col, "more than 64 instructions");
    if (op <= kPushRed) {
      if (++depth_ > kMaxStack) return failb(kBadParam, col, "the operand stack would be deeper than 8: regroup the expression");
      if (depth_ > max_depth_) max_depth_ = depth_;
    } else if (op < kNeg) {
      --depth_;
    }
    Ins& i = stream()[count()++];
    i.op = op;
    i.arg = arg;
    i.value = 0.0f;
    return true;
  }
  bool emit_const(float v, size_t col) {
    if (!emit(kPushConst, 0, col)) return false;
    stream()[count() - 1].value = v;
    return true;
  }
  // drops the last instruction of the stream, a kPushConst (constant folding)
  void unpush() {
    --count();
    --depth_;
  }

  static bool is_alpha(char c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '_'; }
  static bool is_digit(char c) { return c >= '0' && c <= '9'; }

  // expr := term (('+' | '-') term)*
  bool parse_expr(int nest, Node* out) {
    if (nest > kMaxNesting) return failb(kBadParam, pos_, "nested deeper than 64 levels");
    Node a;
    if (!parse_term(nest, &a)) return false;
    for (;;) {
      skip();
      if (at_end() || (s_[pos_] != '+' && s_[pos_] != '-')) break;
      const size_t col = pos_;
      const uint8_t op = s_[pos_] == '+' ? kAdd : kSub;
      ++pos_;
      Node b;
      if (!parse_term(nest, &b)) return false;
      if (!combine(op, a, b, col, &a)) return false;
    }
    *out = a;
    return true;
  }

  // term := unary (('*' | '/' | '.*' | './') unary)*
  bool parse_term(int nest, Node* out) {
    Node a;
    if (!parse_unary(nest, &a)) return false;
    for (;;) {
      skip();
      if (at_end()) break;
      const size_t col = pos_;
      uint8_t op;
      bool dotted = false;
      if (s_[pos_] == '*' || s_[pos_] == '/') {
        op = s_[pos_] == '*' ? kMul : kDiv;
        ++pos_;
      } else if (s_[pos_] == '.' && pos_ + 1 < len_ && (s_[pos_ + 1] == '*' || s_[pos_ + 1] == '/')) {
        op = s_[pos_ + 1] == '*' ? kMul : kDiv;
        dotted = true;
        pos_ += 2;
      } else {
        break;
      }
      Node b;
      if (!parse_unary(nest, &b)) return false;
      if (op == kMul && !dotted && a.map && b.map)
        return failb(kUnsupported, col, "map * map is EigenLab's matrix product, which is not built: write .* for the element-wise product");
      if (!combine(op, a, b, col, &a)) return false;
    }
    *out = a;
    return true;
  }

  // unary := ('-' | '+') unary | power
  bool parse_unary(int nest, Node* out) {
    if (nest > kMaxNesting) return failb(kBadParam, pos_, "nested deeper than 64 levels");
    skip();
    if (!at_end() && (s_[pos_] == '-' || s_[pos_] == '+')) {
      const size_t col = pos_;
      const bool neg = s_[pos_] == '-';
      ++pos_;
      Node a;
      if (!parse_unary(nest + 1, &a)) return false;
      if (neg && !negate(a, col, &a)) return false;
      *out = a;
      return true;
    }
    return parse_power(nest, out);
  }

  // power := primary (('^' | '.^') sign* primary)*   left-associative; -a^2 = -(a^2), 2^-1 allowed
  bool parse_power(int nest, Node* out) {
    Node a;
    if (!parse_primary(nest, &a)) return false;
    for (;;) {
      skip();
      if (at_end()) break;
      const size_t col = pos_;
      bool dotted = false;
      if (s_[pos_] == '^') {
        ++pos_;
      } else if (s_[pos_] == '.' && pos_ + 1 < len_ && s_[pos_ + 1] == '^') {
        dotted = true;
        pos_ += 2;
      } else {
        break;
      }
      bool neg = false;
      for (skip(); !at_end() && (s_[pos_] == '-' || s_[pos_] == '+'); skip()) {
        if (s_[pos_] == '-') neg = !neg;
        ++pos_;
      }
      const size_t ecol = pos_;
      Node b;
      if (!parse_primary(nest, &b)) return false;
      if (neg && !negate(b, ecol, &b)) return false;
      if (!dotted && b.map) return failb(kUnsupported, col, "^ needs a scalar exponent (a matrix power is not built): write .^ for the element-wise power");
      if (!emit(kPow, 0, col)) return false;
      a.map = a.map || b.map;
      a.konst = false;  // (never folded through a function)
    }
    *out = a;
    return true;
  }

  bool negate(const Node& a, size_t col, Node* out) {
    *out = a;
    if (a.konst) {
      unpush();
      out->value = -a.value;
      return emit_const(out->value, col);
    }
    return emit(kNeg, 0, col);
  }

  // a (op) b with both already emitted; two constants fold through + - * /
  bool combine(uint8_t op, const Node& a, const Node& b, size_t col, Node* out) {
    Node r;
    r.map = a.map || b.map;
    if (a.konst && b.konst) {
      unpush();
      unpush();
      volatile float x = a.value, y = b.value;  // (one float32 operation, whatever the host compiler's flags)
      volatile float v = op == kAdd ? x + y : op == kSub ? x - y : op == kMul ? x * y : x / y;
      r.konst = true;
      r.value = v;
      *out = r;
      return emit_const(r.value, col);
    }
    *out = r;
    return emit(op, 0, col);
  }

  // digits [. digits] [e [sign] digits] | . digits [exponent]; "2.*a" is 2 .* a as in MATLAB
  bool parse_number(Node* out) {
    const size_t start = pos_;
    size_t p = pos_;
    bool digits = false;
    while (p < len_ && is_digit(s_[p])) ++p, digits = true;
    if (p < len_ && s_[p] == '.' && !(digits && p + 1 < len_ && (s_[p + 1] == '*' || s_[p + 1] == '/' || s_[p + 1] == '^'))) {
      ++p;
      while (p < len_ && is_digit(s_[p])) ++p, digits = true;
    }
    if (!digits) return failb(kBadParam, start, "a number needs a digit");
    if (p < len_ && (s_[p] == 'e' || s_[p] == 'E')) {
      size_t q = p + 1;
      if (q < len_ && (s_[q] == '-' || s_[q] == '+')) ++q;
      if (q < len_ && is_digit(s_[q])) {
        while (q < len_ && is_digit(s_[q])) ++q;
        p = q;
      }
    }
    if (p < len_ && is_alpha(s_[p])) return failb(kBadParam, p, "unexpected character behind a number");
    if (p - start >= 64) return failb(kBadParam, start, "a number of more than 63 characters");
    char buf[64];
    memcpy(buf, s_ + start, p - start);
    buf[p - start] = 0;
    out->map = false;
    out->konst = true;
    out->value = (float)strtod(buf, nullptr);  // float32(double(text))
    pos_ = p;
    return emit_const(out->value, start);
  }

  struct Fn {
    const char* name;
    int kind;  // 0 unary function, 1 binary function, 2 reduction, 3 valid EigenLab that is not built
    uint8_t code;
  };
  static const Fn* find_fn(const char* s, size_t n) {
    static const Fn k[] = {
        {"abs", 0, kAbs}, {"sqrt", 0, kSqrt}, {"square", 0, kSquare}, {"exp", 0, kExp}, {"log", 0, kLog}, {"log10", 0, kLog10},
        {"sin", 0, kSin}, {"cos", 0, kCos}, {"tan", 0, kTan}, {"asin", 0, kAsin}, {"acos", 0, kAcos},
        {"cwiseMin", 1, kMin}, {"cwiseMax", 1, kMax},
        {"sum", 2, kSum}, {"mean", 2, kMean}, {"sumOfFinites", 2, kSumFinite}, {"meanOfFinites", 2, kMeanFinite},
        {"minOfFinites", 2, kMinFinite}, {"maxOfFinites", 2, kMaxFinite}, {"numberOfFinites", 2, kCountFinite},
        {"min", 3, 0}, {"max", 3, 0}, {"transpose", 3, 0}, {"trace", 3, 0}, {"norm", 3, 0}, {"zeros", 3, 0}, {"ones", 3, 0}, {"eye", 3, 0},
        {"prod", 3, 0}, {"det", 3, 0}, {"inverse", 3, 0}, {"conjugate", 3, 0}, {"adjoint", 3, 0}, {"size", 3, 0}, {"absmax", 3, 0},
        {"cwiseProduct", 3, 0}, {"cwiseQuotient", 3, 0}};
    for (const Fn& f : k)
      if (strlen(f.name) == n && memcmp(f.name, s, n) == 0) return &f;
    return nullptr;
  }

  // a layer by its name: the reference's 15, then the user names handed to compile()
  const LayerName* find_layer(const char* s, size_t n) const {
    int n_ref = 0;
    const LayerName* const ref = layer_names(&n_ref);
    for (int k = 0; k < n_ref + n_user_; ++k) {
      const LayerName* const name = k < n_ref ? &ref[k] : &user_[k - n_ref];
      if (strlen(name->name) == n && memcmp(name->name, s, n) == 0) return name;
    }
    return nullptr;
  }

  // primary := number | '(' expr ')' | layer | function '(' args ')'
  bool parse_primary(int nest, Node* out) {
    if (nest > kMaxNesting) return failb(kBadParam, pos_, "nested deeper than 64 levels");
    skip();
    if (at_end()) return failb(kBadParam, pos_, "the expression ends where an operand is expected");
    const char ch = s_[pos_];
    if (is_digit(ch) || (ch == '.' && pos_ + 1 < len_ && is_digit(s_[pos_ + 1]))) return parse_number(out);
    if (ch == '(') {
      const size_t col = pos_;
      ++pos_;
      if (!parse_expr(nest + 1, out)) return false;
      skip();
      if (at_end() || s_[pos_] != ')') return failb(kBadParam, col, "unbalanced '('");
      ++pos_;
      return true;
    }
    if (ch == '[') return failb(kUnsupported, pos_, "matrix literals are not built");
    if (!is_alpha(ch)) return failb(kBadParam, pos_, ch == ')' ? "an operand is expected before ')'" : "unexpected character");
    const size_t start = pos_;
    while (pos_ < len_ && (is_alpha(s_[pos_]) || is_digit(s_[pos_]))) ++pos_;
    const size_t n = pos_ - start;
    skip();
    const bool call = !at_end() && s_[pos_] == '(';
    if (const LayerName* const name = find_layer(s_ + start, n)) {
      if (call) return failb(kUnsupported, pos_, "indexing into a layer is not built");
      if (window_ && name->id != win_layer_)
        return failb(kBadParam, start, "a window expression has one variable: the input layer, written by its name");
      int slot = 0;
      while (slot < n_layers_ && layer_id_[slot] != name->id) ++slot;
      if (slot == n_layers_) {
        if (n_layers_ >= kMaxLayers) return failb(kBadParam, start, "more than 8 distinct layers");
        layer_id_[n_layers_++] = name->id;
      }
      out->map = true;
      out->konst = false;
      return emit(kPushLayer, (uint8_t)slot, start);
    }
    const Fn* f = find_fn(s_ + start, n);
    if (!f) return failb(kBadParam, start, "unknown name (neither a layer of the map nor a function)");
    if (f->kind == 3) return failb(kUnsupported, start, "this EigenLab function is not built (matrix algebra, and min / max whose NaN behaviour depends on Eigen's version: use minOfFinites / maxOfFinites)");
    if (!call) return failb(kBadParam, pos_, "'(' expected behind a function name");
    const size_t open = pos_;
    ++pos_;
    if (f->kind == 2) {
      if (!window_ && red_depth_ > 0) return failb(kBadParam, start, "reductions do not nest");
      if (red_depth_ > 1) return failb(kBadParam, start, "reductions nest one level at most");
      if (n_red_ >= kMaxRed) return failb(kBadParam, start, "more than 4 reductions");
      const int r = n_red_++;
      red_kind_[r] = f->code;
      ++red_depth_;
      red_stream_[r] = red_depth_;
      red_begin_[r] = count();
      const int saved_depth = depth_;
      depth_ = 0;
      Node a;
      const bool ok = parse_expr(nest + 1, &a) && close_call(open, 1);
      if (ok) red_end_[r] = count();
      --red_depth_;
      depth_ = saved_depth;
      if (!ok) return false;
      red_level_[r] = n_red_ > r + 1 ? 1 : 0;  // (the reductions numbered behind r so far are those of its argument)
      out->map = false;
      out->konst = false;
      return emit(kPushRed, (uint8_t)r, start);
    }
    Node a;
    if (!parse_expr(nest + 1, &a)) return false;
    if (f->kind == 1) {
      skip();
      if (at_end() || s_[pos_] != ',') return failb(kBadParam, pos_, "this function takes two arguments");
      ++pos_;
      Node b;
      if (!parse_expr(nest + 1, &b)) return false;
      a.map = a.map || b.map;
    }
    if (!close_call(open, f->kind == 1 ? 2 : 1)) return false;
    out->map = a.map;
    out->konst = false;  // (never folded through a function)
    return emit(f->code, 0, start);
  }

  bool close_call(size_t open, int arity) {
    skip();
    if (!at_end() && s_[pos_] == ',') return failb(kBadParam, pos_, arity == 1 ? "this function takes one argument" : "this function takes two arguments");
    if (at_end() || s_[pos_] != ')') return failb(kBadParam, open, "unbalanced '('");
    ++pos_;
    return true;
  }
};

inline int compile(const char* text, Program* out, char* err, size_t err_len, const LayerName* user = nullptr, int n_user = 0) {
  return Compiler::compile(text, out, err, err_len, -1, user, n_user);
}

// One ThresholdFilter behind an expression: `lower` -- v < threshold ? set_to : v, otherwise v > threshold ? set_to : v.
struct Threshold {
  bool lower;
  float threshold, set_to;
};
constexpr int kMaxThresholds = 4;

// Appends the n thresholds, in order, to the main code of a compiled program: one instruction and two constants each.  kOk, or
// kBadParam where the program then exceeds the 64 instructions (or its table of constants) -- the caller runs the thresholds as
// passes of their own.  The arguments of the reductions move up behind the longer main code.
inline int append_thresholds(Program* p, int n, const Threshold* t, char* err, size_t err_len) {
  if (err && err_len) err[0] = 0;
  if (n < 0 || n > kMaxThresholds || (n > 0 && !t)) {
    if (err && err_len) snprintf(err, err_len, "expression: %d thresholds (0 .. %d)", n, kMaxThresholds);
    return kBadParam;
  }
  if (p->n_code + n > kMaxCode || p->n_consts + 2 * n > kMaxCode) {
    if (err && err_len) snprintf(err, err_len, "expression: more than 64 instructions with its %d thresholds", n);
    return kBadParam;
  }
  for (int k = p->n_code - 1; k >= p->n_main; --k) {
    p->op[k + n] = p->op[k];
    p->arg[k + n] = p->arg[k];
  }
  for (int k = 0; k < p->n_red; ++k) {
    p->red_begin[k] = (uint8_t)(p->red_begin[k] + n);
    p->red_end[k] = (uint8_t)(p->red_end[k] + n);
  }
  for (int k = 0; k < n; ++k) {
    p->op[p->n_main + k] = t[k].lower ? kThreshLower : kThreshUpper;
    p->arg[p->n_main + k] = (uint8_t)p->n_consts;
    p->consts[p->n_consts++] = t[k].threshold;
    p->consts[p->n_consts++] = t[k].set_to;
  }
  p->n_main += n;
  p->n_code += n;
  return kOk;
}

// window mode: `in_layer` (a te_layer id) is the one variable and denotes the window; the result must be a scalar;
// reductions nest one level
// user / n_user: the context's user layers; `in_layer` may be one of them
inline int compile_window(const char* text, int in_layer, Program* out, char* err, size_t err_len, const LayerName* user = nullptr,
                          int n_user = 0) {
  int n = 0;
  layer_names(&n);
  bool known = in_layer >= 0 && in_layer < n;
  for (int k = 0; user && k < n_user; ++k) known = known || user[k].id == in_layer;
  if (!known) {
    memset(out, 0, sizeof(*out));
    if (err && err_len) snprintf(err, err_len, "expression: bad input layer %d", in_layer);
    return kBadParam;
  }
  return Compiler::compile(text, out, err, err_len, in_layer, user, n_user);
}

inline uint32_t layer_mask(const Program& p) {
  uint32_t m = 0;
  for (int k = 0; k < p.n_layers; ++k) m |= 1u << p.layer_id[k];
  return m;
}

}  // namespace expr
}  // namespace te
