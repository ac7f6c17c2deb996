// components_check.cpp -- the routines of csrc/te_components.h and the plan of csrc/te_components_plan.h on the host.
//   (no argument)            every check below; prints "<n> checks, <k> failed checks"
//   tiles <rows> <cols>      prints "<tiles_i> <tiles_j> <ti> <tj> <seam_cells> <scratch_bytes> <fits> <flat_blocks> <write_blocks>" of
//                            the device's plan
// The labelling runs the headers' own per-lane and per-cell routines under the Plain policy, tile by tile and seam cell by seam
// cell in the order the plan gives, exactly as the kernels of te_components.hip call them.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "te_components.h"
#include "te_components_plan.h"

using namespace te::components;

static long checks = 0, failed = 0;
#define CHECK(cond, ...)                   \
  do {                                     \
    ++checks;                              \
    if (!(cond)) {                         \
      if (++failed <= 20) {                \
        printf("FAILED %s: ", #cond);      \
        printf(__VA_ARGS__);               \
        printf("\n");                      \
      }                                    \
    }                                      \
  } while (0)

// ---- the definition: a flood fill scanned in storage order ----
static void flood(const std::vector<uint8_t>& fr, int rows, int cols, int conn, std::vector<uint32_t>* lab, std::vector<uint32_t>* size) {
  const size_t n = (size_t)rows * cols;
  lab->assign(n, kBlocked);
  size->assign(n, 0);
  std::vector<uint32_t> stack;
  static const int di[8] = {-1, 1, 0, 0, -1, -1, 1, 1}, dj[8] = {0, 0, -1, 1, -1, 1, -1, 1};
  for (size_t x = 0; x < n; ++x) {
    if (!fr[x] || (*lab)[x] != kBlocked) continue;
    (*lab)[x] = (uint32_t)x;
    stack.assign(1, (uint32_t)x);
    uint32_t count = 0;
    while (!stack.empty()) {
      const uint32_t y = stack.back();
      stack.pop_back();
      ++count;
      const int i = (int)(y % rows), j = (int)(y / rows);
      for (int k = 0; k < conn; ++k) {
        const int p = i + di[k], q = j + dj[k];
        if (p < 0 || p >= rows || q < 0 || q >= cols) continue;
        const size_t z = (size_t)q * rows + p;
        if (fr[z] && (*lab)[z] == kBlocked) (*lab)[z] = (uint32_t)x, stack.push_back((uint32_t)z);
      }
    }
    (*size)[x] = count;
  }
}

// ---- the device's launches, on the host ----
static void label_host(const std::vector<uint8_t>& fr, const Plan& p, int conn, bool seams_backwards, std::vector<uint32_t>* Lv, std::vector<uint32_t>* Sv) {
  static uint32_t lab[kTJ * kLanes], cnt[kTJ * kLanes], root[kTJ * kLanes];
  static uint64_t msk[kTJ];
  Lv->assign((size_t)p.cells, 0xdeadbeefu);
  Sv->assign((size_t)p.cells, 0xdeadbeefu);
  uint32_t* L = Lv->data();
  uint32_t* S = Sv->data();
  // (lanes at and behind p.ti hold no cell: their labels are kBlocked and nothing reads them)
  for (unsigned long long b = 0; b < p.tile_blocks; ++b) {
    int i0, j0;
    tile_origin(p, b, &i0, &j0);
    const int nc = p.cols - j0 < p.tj ? p.cols - j0 : p.tj;
    for (int c = 0; c < nc; ++c) {
      uint64_t m = 0;
      for (int l = 0; l < p.ti; ++l)
        if (i0 + l < p.rows && fr[(size_t)(j0 + c) * p.rows + i0 + l]) m |= 1ull << l;
      msk[c] = m;
      for (int l = 0; l < p.ti; ++l) lab[c * kLanes + l] = tile_first_label(m, c, l), cnt[c * kLanes + l] = 0;
    }
    for (int c = 1; c < nc; ++c)
      for (int l = 0; l < p.ti; ++l) tile_unite_lane<Plain>(lab, c, l, msk[c], msk[c - 1], conn);
    for (int c = 0; c < nc; ++c)
      for (int l = 0; l < p.ti; ++l) {
        const uint32_t t = lab[c * kLanes + l];
        root[c * kLanes + l] = kBlocked;
        if (t == kBlocked) continue;
        const uint32_t r = find<Plain>(lab, t);
        root[c * kLanes + l] = r;
        if ((run_starts(msk[c]) >> l) & 1ull) Plain::fetch_add(&cnt[r], (uint32_t)run_length(msk[c], l));
      }
    for (int c = 0; c < nc; ++c)
      for (int l = 0; l < p.ti && i0 + l < p.rows; ++l) {
        const size_t x = (size_t)(j0 + c) * p.rows + i0 + l;
        const uint32_t r = root[c * kLanes + l];
        CHECK(L[x] == 0xdeadbeefu, "cell %zu has two owning tiles", x);
        L[x] = r == kBlocked ? kBlocked : (uint32_t)((size_t)(j0 + (int)(r / kLanes)) * p.rows + (size_t)(i0 + (int)(r % kLanes)));
        S[x] = cnt[c * kLanes + l];
      }
  }
  for (unsigned long long k = 0; k < p.seam_cells; ++k) {
    const unsigned long long u = seams_backwards ? p.seam_cells - 1 - k : k;
    bool col_seam;
    int i, j;
    seam_cell(p, u, &col_seam, &i, &j);
    if (col_seam)
      seam_col_cell<Plain>(L, p.rows, p.ti, i, j, conn);
    else
      seam_row_cell<Plain>(L, p.rows, p.cols, p.tj, i, j, conn);
  }
  for (unsigned long long x = 0; x < p.cells; ++x) flatten_cell<Plain>(L, S, (uint32_t)x);
}

static void check_map(const std::vector<uint8_t>& fr, int rows, int cols, int ti, int tj, const char* what) {
  std::vector<uint32_t> lab, size, L, S;
  for (int conn = 4; conn <= 8; conn += 4) {
    flood(fr, rows, cols, conn, &lab, &size);
    for (int back = 0; back < 2; ++back) {
      const Plan p = plan(rows, cols, 1, ti, tj);
      label_host(fr, p, conn, back != 0, &L, &S);
      bool same = true;
      for (size_t x = 0; x < (size_t)p.cells && same; ++x) {
        same = L[x] == lab[x];
        if (same && lab[x] != kBlocked) same = size_value(L[x], S.data()) == (float)size[lab[x]];
        if (same && lab[x] == kBlocked) same = size_value(L[x], S.data()) == 0.0f && reach_value(L[x], S.data()) == 0.0f;
      }
      CHECK(same, "%s %d x %d, tiles of %d x %d, connectivity %d, seams %s", what, rows, cols, ti, tj, conn, back ? "backwards" : "forwards");
      // a start on the last cell: its component and nothing else
      const size_t s = (size_t)p.cells - 1;
      if (L[s] != kBlocked) Plain::fetch_or(S.data() + L[s], kFlag);
      bool reach = true;
      for (size_t x = 0; x < (size_t)p.cells && reach; ++x) {
        const float want = lab[x] != kBlocked && lab[x] == lab[s] ? 1.0f : 0.0f;
        reach = reach_value(L[x], S.data()) == want && size_value(L[x], S.data()) == (lab[x] == kBlocked ? 0.0f : (float)size[lab[x]]);
      }
      CHECK(reach, "reachable: %s %d x %d, tiles of %d x %d, connectivity %d", what, rows, cols, ti, tj, conn);
    }
  }
}

static void check_runs(uint64_t m) {
  for (int l = 0; l < 64; ++l) {
    if (!((m >> l) & 1ull)) continue;
    int s = l;
    while (s > 0 && ((m >> (s - 1)) & 1ull)) --s;
    int e = l;
    while (e < 63 && ((m >> (e + 1)) & 1ull)) ++e;
    CHECK(run_start(m, l) == s, "run_start(%llx, %d) = %d, want %d", (unsigned long long)m, l, run_start(m, l), s);
    CHECK(run_length(m, l) == e - l + 1, "run_length(%llx, %d) = %d, want %d", (unsigned long long)m, l, run_length(m, l), e - l + 1);
    CHECK((int)((run_starts(m) >> l) & 1ull) == (s == l), "run_starts(%llx) bit %d", (unsigned long long)m, l);
  }
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

static void check_plan(int rows, int cols, int ti, int tj) {
  const Plan p = plan(rows, cols, 3, ti, tj);
  std::vector<int> owner((size_t)rows * cols, 0), seam((size_t)rows * cols, 0);
  for (unsigned long long b = 0; b < p.tile_blocks; ++b) {
    int i0, j0;
    tile_origin(p, b, &i0, &j0);
    for (int j = j0; j < j0 + tj && j < cols; ++j)
      for (int i = i0; i < i0 + ti && i < rows; ++i) ++owner[(size_t)j * rows + i];
  }
  for (unsigned long long u = 0; u < p.seam_cells; ++u) {
    bool col_seam;
    int i, j;
    seam_cell(p, u, &col_seam, &i, &j);
    CHECK(i >= 0 && i < rows && j >= 0 && j < cols, "seam cell %llu of %d x %d lies outside", u, rows, cols);
    CHECK(col_seam ? (j >= 1 && j % tj == 0) : (i >= 1 && i % ti == 0), "seam cell %llu of %d x %d is on no seam", u, rows, cols);
    if (i >= 0 && i < rows && j >= 0 && j < cols) seam[(size_t)j * rows + i] += col_seam ? 1 : 16;
  }
  bool one_owner = true, seams_once = true;
  for (int j = 0; j < cols; ++j)
    for (int i = 0; i < rows; ++i) {
      one_owner = one_owner && owner[(size_t)j * rows + i] == 1;
      const int want = (j >= 1 && j % tj == 0 ? 1 : 0) + (i >= 1 && i % ti == 0 ? 16 : 0);
      seams_once = seams_once && seam[(size_t)j * rows + i] == want;
    }
  CHECK(one_owner, "%d x %d, tiles of %d x %d: a cell without exactly one owning tile", rows, cols, ti, tj);
  CHECK(seams_once, "%d x %d, tiles of %d x %d: a seam cell not visited exactly once", rows, cols, ti, tj);
  CHECK(p.scratch_bytes == (size_t)rows * cols * 3 * 8, "scratch of %d x %d", rows, cols);
  CHECK(p.seam_blocks * kThreads >= p.seam_cells && p.flat_blocks * kThreads >= p.cells && p.write_blocks >= 1 && p.fits, "grids of %d x %d", rows, cols);
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "tiles")) {
    const Plan p = plan(atoi(argv[2]), atoi(argv[3]), 1);
    printf("%u %u %d %d %llu %zu %d %llu %u\n", p.tiles_i, p.tiles_j, p.ti, p.tj, p.seam_cells, p.scratch_bytes, p.fits ? 1 : 0, p.flat_blocks, p.write_blocks);
    return 0;
  }
  // runs of a mask: every mask of a 12-bit chunk at three places of the word, and random words
  for (uint64_t m = 0; m < 4096; ++m) check_runs(m), check_runs(m << 26), check_runs(m << 52), check_runs(~m);
  for (int k = 0; k < 2000; ++k) check_runs(rnd()), check_runs(rnd() & rnd()), check_runs(rnd() | rnd());
  check_runs(~0ull);
  // link_masks: one union per overlap of two runs, and the diagonals that no straight step covers
  for (int k = 0; k < 20000; ++k) {
    const uint64_t m = k < 4096 ? (uint64_t)k : rnd() & rnd(), p = k < 4096 ? (uint64_t)(k * 2654435761u) >> 20 : rnd() & rnd();
    uint64_t d, u, dn, d8, u4, dn4;
    link_masks(m, p, 8, &d, &u, &dn);
    link_masks(m, p, 4, &d8, &u4, &dn4);
    bool ok = d == d8 && u4 == 0 && dn4 == 0;
    for (int l = 0; l < 64 && ok; ++l) {
      const auto bit = [](uint64_t w, int b) { return b >= 0 && b < 64 && ((w >> b) & 1ull); };
      ok = bit(d, l) == (bit(m, l) && bit(p, l) && !(bit(m, l - 1) && bit(p, l - 1))) &&
           bit(u, l) == (bit(m, l) && bit(p, l - 1) && !bit(p, l) && !bit(m, l - 1)) &&
           bit(dn, l) == (bit(m, l) && bit(p, l + 1) && !bit(p, l) && !bit(m, l + 1));
    }
    CHECK(ok, "link_masks(%llx, %llx)", (unsigned long long)m, (unsigned long long)p);
  }
  // every binary map up to 4 x 4 with tile edges forced down to 2 and 3 cells, and the device's own
  static const int edges[5][2] = {{2, 2}, {3, 3}, {2, 3}, {3, 2}, {kTI, kTJ}};
  for (int rows = 1; rows <= 4; ++rows)
    for (int cols = 1; cols <= 4; ++cols) {
      std::vector<uint8_t> fr((size_t)rows * cols);
      for (uint32_t bitsv = 0; bitsv < (1u << (rows * cols)); ++bitsv) {
        for (int x = 0; x < rows * cols; ++x) fr[x] = (bitsv >> x) & 1u;
        for (const auto& e : edges) check_map(fr, rows, cols, e[0], e[1], "every map");
      }
    }
  // larger random maps over several tiles, the percolation threshold among the densities
  static const int shapes[6][2] = {{7, 9}, {13, 5}, {70, 70}, {130, 67}, {5, 300}, {200, 3}};
  static const double dens[4] = {0.3, 0.5, 0.593, 0.8};
  for (const auto& s : shapes)
    for (const double d : dens) {
      std::vector<uint8_t> fr((size_t)s[0] * s[1]);
      for (auto& v : fr) v = (double)(rnd() >> 11) / 9007199254740992.0 < d;
      check_map(fr, s[0], s[1], kTI, kTJ, "random");
      check_map(fr, s[0], s[1], 3, 2, "random");
      check_map(fr, s[0], s[1], 5, 7, "random");
    }
  // the plan: owners and seams
  static const int pshapes[7][2] = {{1, 1}, {1, 9}, {9, 1}, {70, 70}, {130, 67}, {577, 6}, {5, 300}};
  for (const auto& s : pshapes) {
    check_plan(s[0], s[1], kTI, kTJ);
    check_plan(s[0], s[1], 2, 3);
    check_plan(s[0], s[1], 3, 2);
  }
  CHECK(!plan(65536, 32768, 1).fits && plan(46340, 46340, 1).fits, "the limit of 2^31 cells");
  printf("%ld checks, %ld failed checks\n", checks, failed);
  return failed ? 1 : 0;
}
