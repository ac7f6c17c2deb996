// expr_user_check.cpp -- the CPU build of the expression compiler and evaluator (te_expr.h) with user layer names, and the two
// threshold opcodes append_thresholds() puts behind a program (tests/test_expr_user_names.py).
//   info  NAMES TEXT                     NAMES: comma-separated user names, added in order (te_user_layers.h); prints
//                                        "rc=.. mask=0x.. code=.. main=.. err=.."
//   add   NAME                           prints the status of user::Table::add
//   eval  NAMES TEXT N (l|u):T:S ... -- BITS ...
//                                        compiles TEXT (one operand: the first user name), appends the N thresholds (T, S: float
//                                        bit patterns in hex) and evaluates it for every input value (hex bit patterns); prints
//                                        "rc=.." and the results' bit patterns in hex
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "te_user_layers.h"

using namespace te;

static float from_bits(const char* hex) {
  const uint32_t u = (uint32_t)strtoul(hex, nullptr, 16);
  float f;
  memcpy(&f, &u, 4);
  return f;
}

static int add_names(user::Table& t, const char* csv) {
  std::string s(csv);
  size_t at = 0;
  while (at < s.size()) {
    const size_t end = s.find(',', at) == std::string::npos ? s.size() : s.find(',', at);
    const std::string name = s.substr(at, end - at);
    int id = -1;
    const char* why = "";
    if (!name.empty() && t.add(name.c_str(), &id, &why) != TE_OK) {
      printf("add '%s': %s\n", name.c_str(), why);
      return 1;
    }
    at = end + 1;
  }
  return 0;
}

struct Stack1 {
  expr::Vec<1> s[expr::kMaxStack];
  void put(int k, const expr::Vec<1>& v) { s[k] = v; }
  expr::Vec<1> get(int k) const { return s[k]; }
};
struct Source1 {
  float x;
  expr::Vec<1> layer(int) const { return expr::Vec<1>{{x}}; }
  expr::Vec<1> red(int) const { return expr::Vec<1>{{0.0f}}; }
};

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const std::string cmd = argv[1];
  user::Table t;
  if (cmd == "add") {
    int id = -1;
    const char* why = "";
    const int rc = t.add(argv[2], &id, &why);
    printf("rc=%d id=%d why=%s\n", rc, id, why);
    return 0;
  }
  if (argc < 4 || add_names(t, argv[2])) return 2;
  expr::LayerName ops[user::kMax];
  const int n_ops = t.operands(ops);
  expr::Program p;
  char err[200];
  int rc = expr::compile(argv[3], &p, err, sizeof(err), ops, n_ops);
  if (cmd == "info") {
    printf("rc=%d mask=0x%x code=%d main=%d err=%s\n", rc, rc == expr::kOk ? expr::layer_mask(p) : 0u, p.n_code, p.n_main, err);
    return 0;
  }
  if (cmd != "eval" || argc < 5) return 2;
  const int n = atoi(argv[4]);
  std::vector<expr::Threshold> th;
  int k = 5;
  for (; k < argc && (int)th.size() < n; ++k) {
    char mode = 0, a[32], b[32];
    if (sscanf(argv[k], "%c:%31[^:]:%31s", &mode, a, b) != 3) return 2;
    th.push_back(expr::Threshold{mode == 'l', from_bits(a), from_bits(b)});
  }
  if (k >= argc || strcmp(argv[k], "--") != 0) return 2;
  if (rc == expr::kOk) rc = expr::append_thresholds(&p, n, th.data(), err, sizeof(err));
  printf("rc=%d code=%d main=%d err=%s\n", rc, p.n_code, p.n_main, err);
  if (rc != expr::kOk) return 0;
  for (++k; k < argc; ++k) {
    Stack1 st;
    const Source1 src{from_bits(argv[k])};
    const float v = expr::run<1>(p, 0, p.n_main, st, src).v[0];
    uint32_t u;
    memcpy(&u, &v, 4);
    printf("%08x\n", u);
  }
  return 0;
}
