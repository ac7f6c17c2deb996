// te_slab.h -- the layout of a context's slab (te_set_geometry's one allocation) as a plan: plain C++, shared with the
// CPU test (tests/cpu/slab_plan_check.cpp).  The marching kernels of te_march5.h load kSlabGuardRows rows above and below
// the layers they are given, unconditionally; that those rows exist is this layout and nothing else.
//
// The parts, in memory order, each starting on a 256-byte boundary and contiguous:
//   front guard | 13 float layers | mask bytes | fix-up flags | blocked list | its counter block | untraversable flags |
//   sum scratch | face flags | back guard
#pragma once
#include <stddef.h>

namespace te {

// rows of slack before the first and behind the last part that kernels read: the largest stencil radius (kMaxRadiusCells)
// plus the marches' prefetch distance of 16 (te_internal.h holds the two together)
constexpr int kSlabGuardRows = 48;
constexpr int kSlabFloatLayers = 13;

// Beside the slab: the scratch of te_move_map (te_move.hip), one float layer of ONE map whatever the batch.  It is a buffer of
// its own (te_ctx::LayerMem::move_scratch), allocated by the first move and freed with the slab: no kernel marches over it, so
// it needs no guard rows, and contexts that never move do not pay for it.
inline size_t move_scratch_bytes(int rows, int cols) { return (size_t)rows * (size_t)cols * sizeof(float); }

struct SlabPart {
  size_t off, bytes;
};

struct SlabPlan {
  SlabPart front_guard, layers, mask, fix_flags, list, list_count, untrav_flags, sum_scratch, face_flags, back_guard;
  size_t layer_bytes;  // one float layer of `layers`
  size_t list_cap;     // entries of the blocked list (and of the sum scratch): one per cell + list_slack
  size_t total;
  size_t layer_off(int k) const { return layers.off + (size_t)k * layer_bytes; }
};

// fix_flag_count: fast::normals_fast_max_blocks (ints); list_slack: fast::fp_list_slack (entries beyond one per cell);
// untrav_flag_bytes / face_flag_bytes: the two flag grids (one byte per 64 x 4 cells)
inline SlabPlan plan_slab(int rows, int cols, int batch, size_t fix_flag_count, size_t list_slack, size_t untrav_flag_bytes,
                          size_t face_flag_bytes) {
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t elems = (size_t)rows * (size_t)cols * (size_t)batch;
  const size_t guard = up((size_t)kSlabGuardRows * (size_t)rows * sizeof(float));
  SlabPlan p;
  p.layer_bytes = up(elems * sizeof(float));
  p.list_cap = elems + list_slack;
  size_t at = 0;
  auto part = [&at](size_t bytes) {
    const SlabPart s = {at, bytes};
    at += bytes;
    return s;
  };
  p.front_guard = part(guard);
  p.layers = part(kSlabFloatLayers * p.layer_bytes);
  p.mask = part(up(elems));
  p.fix_flags = part(up(fix_flag_count * sizeof(int)));
  p.list = part(up(p.list_cap * sizeof(unsigned)));
  p.list_count = part(256);
  p.untrav_flags = part(up(untrav_flag_bytes));
  p.sum_scratch = part(p.list.bytes);  // (a second array of the list's size, see Layers::fp_scratch)
  p.face_flags = part(up(face_flag_bytes));
  p.back_guard = part(guard);
  p.total = at;
  return p;
}

}  // namespace te
