// CPU harness over te_path_visit.h (the plan of te_check_footprint_paths_radius), built with the host compiler by
// tests/test_path_visit.py.
//   path_visit_check visit < request   the centres of every path in order, its status, the count formula; then the totals
//       request: rows cols res pos_x pos_y / n_paths / per path: n_poses radius x y x y ...
//       output:  per path "status formula_count n i j i j ..."; last line "stats n_visits n_discs n_classes"
//   path_visit_check keys              pack_key / key_class / key_cell / hash_key / table_entries on the extremes
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>
#include <vector>

#include "te_path_visit.h"

using namespace te;

static int visit_mode() {
  pv::Geom g;
  double res, px, py;
  int n_paths;
  if (scanf("%d %d %lf %lf %lf %d", &g.rows, &g.cols, &res, &px, &py, &n_paths) != 6) return 2;
  g.res = res;
  g.len_x = (double)g.rows * res;
  g.len_y = (double)g.cols * res;
  g.pos_x = px;
  g.pos_y = py;
  std::vector<std::vector<double>> xy(n_paths);
  std::vector<double> radius(n_paths > 0 ? n_paths : 1);
  for (int k = 0; k < n_paths; ++k) {
    int n;
    if (scanf("%d %lf", &n, &radius[k]) != 2) return 2;
    xy[k].resize(2 * (size_t)n);
    for (double& v : xy[k])
      if (scanf("%lf", &v) != 1) return 2;
  }
  std::vector<double> uniq;
  std::vector<int> cls;
  pv::class_radii(n_paths, radius.data(), &uniq, &cls);
  std::vector<uint64_t> keys;
  long long n_visits = 0;
  std::string line;
  for (int k = 0; k < n_paths; ++k) {
    const int n = (int)(xy[k].size() / 2);
    std::vector<int> cells;
    const int st = pv::visit_path(g, n, xy[k].data(), [&](int i, int j) {
      cells.push_back(i);
      cells.push_back(j);
      keys.push_back(pv::pack_key((unsigned)cls[k], i, j, g.rows));
    });
    n_visits += (long long)(cells.size() / 2);
    printf("%d %lld %zu", st, pv::count_path_visits(g, n, xy[k].data()), cells.size() / 2);
    for (int v : cells) printf(" %d", v);
    printf("\n");
  }
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  for (uint64_t key : keys) {  // every key unpacks to a class of the request and a cell of the map
    if (pv::key_class(key) >= uniq.size() || pv::key_cell(key) >= (uint64_t)g.rows * g.cols || key == pv::kEmptyKey) return 3;
  }
  printf("stats %lld %zu %zu\n", n_visits, keys.size(), uniq.size());
  return 0;
}

static int keys_mode() {
  int failed = 0;
  auto check = [&](bool ok, const char* what) {
    if (!ok) {
      ++failed;
      printf("FAILED: %s\n", what);
    }
  };
  // injective up to 32768^2 cells and 2^16 classes: the corners of every factor, and a pseudo-random sample
  const int sizes[][2] = {{1, 1}, {300, 260}, {4096, 4096}, {32768, 32768}, {32768, 7}, {5, 32768}};
  for (const auto& sz : sizes) {
    const int rows = sz[0], cols = sz[1];
    std::set<uint64_t> seen;
    size_t n = 0;
    uint64_t x = 88172645463325252ull;
    auto rnd = [&]() {
      x ^= x << 13;
      x ^= x >> 7;
      x ^= x << 17;
      return x;
    };
    auto one = [&](unsigned c, int i, int j) {
      const uint64_t key = pv::pack_key(c, i, j, rows);
      check(key != pv::kEmptyKey, "a key equals the empty marker");
      check(pv::key_class(key) == c, "class does not round-trip");
      check(pv::key_cell(key) == (uint64_t)j * rows + i, "cell does not round-trip");
      check((int)(pv::key_cell(key) % rows) == i && (int)(pv::key_cell(key) / rows) == j, "(i, j) does not round-trip");
      seen.insert(key);
      ++n;
    };
    const unsigned cs[] = {0u, 1u, 65534u, 65535u};
    for (unsigned c : cs)
      for (int i : {0, rows - 1})
        for (int j : {0, cols - 1}) one(c, i, j);
    std::set<uint64_t> triples;
    for (int k = 0; k < 200000; ++k) {
      const unsigned c = (unsigned)(rnd() % 65536);
      const int i = (int)(rnd() % rows), j = (int)(rnd() % cols);
      triples.insert(((uint64_t)c << 40) | ((uint64_t)i << 20) | (uint64_t)j);  // (20 bits hold 32767)
      one(c, i, j);
    }
    // as many distinct keys as distinct (class, i, j)
    std::set<uint64_t> corner;
    for (unsigned c : cs)
      for (int i : {0, rows - 1})
        for (int j : {0, cols - 1}) corner.insert(((uint64_t)c << 40) | ((uint64_t)i << 20) | (uint64_t)j);
    for (uint64_t t : corner) triples.insert(t);
    check(seen.size() == triples.size(), "two (class, cell) share a key");
  }
  // the table: a power of two, at most half full, never empty
  for (uint64_t v : {0ull, 1ull, 31ull, 32ull, 33ull, 1000ull, 1048576ull, 1048577ull, 1ull << 30}) {
    const uint64_t cap = pv::table_entries(v);
    check(cap >= 64 && (cap & (cap - 1)) == 0 && cap >= 2 * v && (cap == 64 || cap < 4 * v), "table_entries");
  }
  // the hash spreads neighbouring cells of one class over a small table
  {
    std::vector<int> load(1024, 0);
    for (int i = 0; i < 512; ++i) load[pv::hash_key(pv::pack_key(3, i, 17, 4096)) & 1023]++;
    int worst = 0;
    for (int v : load) worst = v > worst ? v : worst;
    check(worst <= 6, "hash_key piles a line of cells into one slot");
  }
  printf("%d failed checks\n", failed);
  return failed ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "visit")) return visit_mode();
  if (argc >= 2 && !strcmp(argv[1], "keys")) return keys_mode();
  fprintf(stderr, "usage: path_visit_check visit|keys\n");
  return 2;
}
