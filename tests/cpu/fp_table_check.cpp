// Prints the tables of te_fp_table.h for one footprint, for tests/test_fp_table.py to hold against the oracle's
// SpiralIterator.  Usage: fp_table_check rmax res rows cols clip
// Output: "reach R n_runs n_ties n_spiral n_spiral_full", then one line of run half-widths, one line of tie offsets
// (di dj pairs) and one line per spiral entry "di dj ring tie".
// fp_table_check pack rmax res: the unclipped spiral packed as the kernels of reach <= 20 read it (fp_pack), decoded as they
// decode it; prints "n_spiral reach mismatches".
#include <cstdio>
#include <cstdlib>
#include <string>

#include "te_fp_table.h"

int main(int argc, char** argv) {
  if (argc == 4 && std::string(argv[1]) == "pack") {
    te::FpTable t;
    te::build_fp_table(atof(argv[2]), atof(argv[3]), 1, 1, &t, false);
    int bad = 0;
    for (const te::FpEntry& e : t.spiral) {
      const uint32_t w = te::fp_pack(e);  // (the kernels: signed bytes di, dj; ring and tie unsigned)
      const int di = (signed char)(w & 0xffu), dj = (signed char)((w >> 8) & 0xffu), ring = (int)((w >> 16) & 0xffu), tie = (int)(w >> 24);
      bad += di != e.di || dj != e.dj || ring != e.ring || tie != e.tie;
    }
    printf("%zu %d %d\n", t.spiral.size(), t.reach, bad);
    return 0;
  }
  if (argc != 6) {
    fprintf(stderr, "usage: %s rmax res rows cols clip\n", argv[0]);
    return 2;
  }
  te::FpTable t;
  te::build_fp_table(atof(argv[1]), atof(argv[2]), atoi(argv[3]), atoi(argv[4]), &t, atoi(argv[5]) != 0);
  printf("%d %d %zu %zu %zu %lld\n", t.reach, t.R, t.hw.size(), t.ties.size() / 2, t.spiral.size(), t.n_spiral_full);
  for (size_t k = 0; k < t.hw.size(); ++k) printf("%d ", t.hw[k]);
  printf("\n");
  for (size_t k = 0; k < t.ties.size(); ++k) printf("%d ", t.ties[k]);
  printf("\n");
  for (const te::FpEntry& e : t.spiral) printf("%d %d %d %d\n", e.di, e.dj, e.ring, e.tie);
  return 0;
}
