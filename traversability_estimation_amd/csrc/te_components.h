// te_components.h -- the per-run and union routines of te_run_components / te_run_reachable (include/travgpu.h: the connected
// regions of the free cells): plain C++ that compiles for the host and the device.  The kernels (te_components.hip) instantiate
// exactly this code, and the CPU test (tests/cpu/components_check.cpp) runs it, tile by tile, against a flood fill.
//
// Layers are column-major: cell (i, j) of a map is element j * rows + i.  A label is the linear index of a cell of the same
// component, never larger than the cell's own: L[x] <= x, and L[x] == x exactly at a root.  Labels only ever decrease, so a
// chain x, L[x], L[L[x]], ... is strictly decreasing and ends at a root; a value read late is an older, larger ancestor of the
// same component and leads to the same root.
//   tile pass    the free cells of 64 rows of a column are one 64-bit mask; a run of set bits is labelled with its first cell
//                (run_start), and runs of neighbouring columns are united once per overlap (link_masks), not once per cell;
//   seam pass    a cell on a tile border unites with its neighbours across the border under the same economy
//                (seam_col_cell, seam_row_cell);
//   flatten      every cell takes its root, and a tile-local root hands its count to the root (flatten_cell).
// Memory is reached through a policy P: relaxed atomics on the device (Atomic<scope>), plain accesses on the host (Plain).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "te_distance.h"

namespace te {
namespace components {

constexpr uint32_t kBlocked = 0xffffffffu;  // the label of a blocked cell
constexpr uint32_t kFlag = 0x80000000u;     // or-ed into the size at a root that holds a start (sizes are below 2^31)

// the host's policy (and the model of the device's: one access each)
struct Plain {
  static inline uint32_t load(const uint32_t* p) { return *p; }
  static inline void store(uint32_t* p, uint32_t v) { *p = v; }
  static inline uint32_t fetch_min(uint32_t* p, uint32_t v) {
    const uint32_t old = *p;
    if (v < old) *p = v;
    return old;
  }
  static inline uint32_t fetch_add(uint32_t* p, uint32_t v) {
    const uint32_t old = *p;
    *p = old + v;
    return old;
  }
  static inline uint32_t fetch_or(uint32_t* p, uint32_t v) {
    const uint32_t old = *p;
    *p = old | v;
    return old;
  }
};

#if defined(__HIPCC__)
// relaxed integer atomics at `kScope` (__HIP_MEMORY_SCOPE_AGENT on what workgroups share, _WORKGROUP on LDS)
template <int kScope>
struct Atomic {
  static __device__ inline uint32_t load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, kScope); }
  static __device__ inline void store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, kScope); }
  static __device__ inline uint32_t fetch_min(uint32_t* p, uint32_t v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, kScope); }
  static __device__ inline uint32_t fetch_add(uint32_t* p, uint32_t v) { return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, kScope); }
  static __device__ inline uint32_t fetch_or(uint32_t* p, uint32_t v) { return __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, kScope); }
};
#endif

// a free cell is one that te_run_distance would not seed: the one predicate (te_distance.h)
TE_DIST_HD bool is_free(float v, int mode, float threshold) { return !distance::is_seed(v, mode, threshold); }

// ---- runs of a 64-bit mask (bit l: row l of the chunk is free) ----
// the first bit of the run that holds bit l (bit l is set)
TE_DIST_HD int run_start(uint64_t m, int l) {
  const uint64_t below = ~m & ((1ull << l) - 1ull);  // the clear bits under l
  return below ? 64 - __builtin_clzll(below) : 0;
}
// the number of set bits from bit l upward without a gap (bit l is set)
TE_DIST_HD int run_length(uint64_t m, int l) {
  const uint64_t gap = ~(m >> l);  // bit 0 clear; the bits shifted in at the top are set, except for l == 0
  return gap ? __builtin_ctzll(gap) : 64;
}
// the first bits of the runs of m
TE_DIST_HD uint64_t run_starts(uint64_t m) { return m & ~(m << 1); }

// The unions between column c (mask m) and the column before it (mask p) of one chunk: bit l of
//   *direct  unite (l, c) with (l, c - 1): the first row of every overlap of a run of m with a run of p;
//   *up      unite (l, c) with (l - 1, c - 1), *down with (l + 1, c - 1) (8-connectivity only): the diagonals no chain of
//            straight steps already covers -- (l, c - 1) is blocked, and so is the cell beside (l, c) in the diagonal's row.
TE_DIST_HD void link_masks(uint64_t m, uint64_t p, int connectivity, uint64_t* direct, uint64_t* up, uint64_t* down) {
  const uint64_t o = m & p;
  *direct = o & ~(o << 1);
  if (connectivity == 8) {
    *up = m & (p << 1) & ~p & ~(m << 1);
    *down = m & (p >> 1) & ~p & ~(m >> 1);
  } else {
    *up = *down = 0;
  }
}

// ---- union-find over an array of labels ----
// Walks a chain of strictly decreasing labels: L[x] <= x, with equality at a root only.  (p >= x ends the walk as well, so the
// loop is bounded by x whatever the array holds.)
template <class P>
TE_DIST_HD uint32_t find(const uint32_t* L, uint32_t x) {
  for (;;) {
    const uint32_t p = P::load(L + x);
    if (p >= x) return x;
    x = p;
  }
}
// find, then x's own entry is lowered to the root: later walks through x are one step long
template <class P>
TE_DIST_HD uint32_t find_compress(uint32_t* L, uint32_t x) {
  const uint32_t r = find<P>(L, x);
  if (r != x) P::fetch_min(L + x, r);
  return r;
}
// Unites the sets of a and b: the larger root's entry is lowered to the smaller root.  Retries an atomic that strictly
// lowered a value: when the entry of `a` was no root any more, the atomic returned its parent `old` < a, the entry is now
// min(old, b), and what is left to unite is `old` and b -- so a + b falls with every turn and the loop ends.
template <class P>
TE_DIST_HD void unite(uint32_t* L, uint32_t a, uint32_t b) {
  a = find_compress<P>(L, a);
  b = find_compress<P>(L, b);
  while (a != b) {
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    const uint32_t old = P::fetch_min(L + a, b);
    if (old == a) return;  // a was a root and hangs under b now
    a = find<P>(L, old);
    b = find<P>(L, b);
  }
}

// ---- the tile pass, per lane: lab holds 64 labels per column of the tile, the label of (l, c) is c * 64 + l ----
constexpr int kLanes = 64;
// the label a cell starts with: the first cell of its run, or kBlocked
TE_DIST_HD uint32_t tile_first_label(uint64_t m, int c, int l) { return (m >> l) & 1ull ? (uint32_t)(c * kLanes + run_start(m, l)) : kBlocked; }
// the unions of lane l of column c >= 1 (m: its mask, p: the mask of column c - 1)
template <class P>
TE_DIST_HD void tile_unite_lane(uint32_t* lab, int c, int l, uint64_t m, uint64_t p, int connectivity) {
  uint64_t direct, up, down;
  link_masks(m, p, connectivity, &direct, &up, &down);
  const uint32_t x = (uint32_t)(c * kLanes + l), a = x - kLanes;
  if ((direct >> l) & 1ull) unite<P>(lab, x, a);
  if ((up >> l) & 1ull) unite<P>(lab, x, a - 1);
  if ((down >> l) & 1ull) unite<P>(lab, x, a + 1);
}

// ---- the seam pass, per cell: L holds one map, ti / tj are the tile edges ----
template <class P>
TE_DIST_HD bool free_at(const uint32_t* L, size_t x) {
  return P::load(L + x) != kBlocked;
}
// Cell (i, j), j >= 1 the first column of a tile, against column j - 1.  Straight: only the first row of an overlap inside one
// tile (the rows before it are the same two tile-local components).  Diagonals as in link_masks.
template <class P>
TE_DIST_HD void seam_col_cell(uint32_t* L, int rows, int ti, int i, int j, int connectivity) {
  const size_t x = (size_t)j * rows + i, a = x - rows;
  if (!free_at<P>(L, x)) return;
  if (free_at<P>(L, a)) {
    if (i % ti == 0 || !(free_at<P>(L, x - 1) && free_at<P>(L, a - 1))) unite<P>(L, (uint32_t)x, (uint32_t)a);
  } else if (connectivity == 8) {
    if (i > 0 && free_at<P>(L, a - 1) && !free_at<P>(L, x - 1)) unite<P>(L, (uint32_t)x, (uint32_t)(a - 1));
    if (i + 1 < rows && free_at<P>(L, a + 1) && !free_at<P>(L, x + 1)) unite<P>(L, (uint32_t)x, (uint32_t)(a + 1));
  }
}
// Cell (i, j), i >= 1 the first row of a tile, against row i - 1
template <class P>
TE_DIST_HD void seam_row_cell(uint32_t* L, int rows, int cols, int tj, int i, int j, int connectivity) {
  const size_t x = (size_t)j * rows + i, b = x - 1;
  if (!free_at<P>(L, x)) return;
  if (free_at<P>(L, b)) {
    if (j % tj == 0 || !(free_at<P>(L, x - rows) && free_at<P>(L, b - rows))) unite<P>(L, (uint32_t)x, (uint32_t)b);
  } else if (connectivity == 8) {
    if (j > 0 && free_at<P>(L, b - rows) && !free_at<P>(L, x - rows)) unite<P>(L, (uint32_t)x, (uint32_t)(b - rows));
    if (j + 1 < cols && free_at<P>(L, b + rows) && !free_at<P>(L, x + rows)) unite<P>(L, (uint32_t)x, (uint32_t)(b + rows));
  }
}

// ---- flatten + count, per cell: S holds the cells of every tile-local component at its tile-local root, 0 elsewhere ----
// The cell takes its root; a tile-local root that is no root hands its count on.  Roots stay roots during this pass, nobody
// adds to the count of a cell that is none, and an entry of L read late still leads to the same root.
template <class P>
TE_DIST_HD void flatten_cell(uint32_t* L, uint32_t* S, uint32_t x) {
  const uint32_t t = P::load(L + x);
  if (t == kBlocked) return;
  const uint32_t r = find<P>(L, t);
  if (r != t) P::store(L + x, r);
  if (r != x) {
    const uint32_t n = P::load(S + x);
    if (n) P::fetch_add(S + r, n);
  }
}

// ---- the outputs of a cell (after flatten: L[x] is the root) ----
TE_DIST_HD float size_value(uint32_t label, const uint32_t* S) { return label == kBlocked ? 0.0f : (float)(S[label] & ~kFlag); }
TE_DIST_HD float reach_value(uint32_t label, const uint32_t* S) { return label != kBlocked && (S[label] & kFlag) ? 1.0f : 0.0f; }

}  // namespace components
}  // namespace te
