// CPU check of the slab plan (traversability_estimation_amd/csrc/te_slab.h), the layout of the one allocation that holds a
// context's layers: te_set_geometry allocates plan.total and takes every pointer and memset range from the plan's parts,
// and the marching kernels read kSlabGuardRows rows beyond the layers without a bounds check.  For every shape:
//   - every part starts on a 256-byte boundary;
//   - the parts come in the stated order, contiguous (hence disjoint), and the total is the end of the back guard;
//   - at least kSlabGuardRows * rows * 4 bytes lie before the first float layer and behind the last part kernels are given;
//   - the total and every offset equal the expressions te_set_geometry summed by hand before the plan existed, restated
//     below (expected()), NOT computed through te_slab.h.
// The two inputs the caller computes on the device side (the fix-up flag count, the list slack) are given values of the
// size the shim passes, and arbitrary ones in the sweep.
//   slab_plan_check [n_random seed]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "te_face_flags.h"
#include "te_fp_route.h"
#include "te_slab.h"

namespace {

int g_failed = 0;
#define CHECK(cond, ...)                   \
  do {                                     \
    if (!(cond)) {                         \
      ++g_failed;                          \
      if (g_failed <= 20) {                \
        printf("FAILED %s: ", #cond);      \
        printf(__VA_ARGS__);               \
        printf("\n");                      \
      }                                    \
    }                                      \
  } while (0)

// the offsets te_set_geometry used: the slab base is 0
struct Expected {
  size_t layer[13], untrav, block_flags, fp_blocked, fp_blocked_count, untrav_flags, fp_scratch, face_flags, back_guard, total;
  size_t lb, ub, fb, qb, ufb, ffb, guard, list_cap, first_memset_bytes;
};

Expected expected(int rows, int cols, int batch, size_t fix_flag_count, size_t list_slack, size_t untrav_bytes, size_t face_bytes) {
  Expected x;
  const size_t elems = (size_t)rows * cols * batch;
  const size_t lb = (elems * sizeof(float) + 255) & ~(size_t)255;
  const size_t ub = (elems + 255) & ~(size_t)255;
  const size_t fb = (fix_flag_count * sizeof(int) + 255) & ~(size_t)255;
  const size_t list_cap = elems + list_slack;
  const size_t qb = (list_cap * sizeof(unsigned) + 255) & ~(size_t)255;
  const size_t guard = ((size_t)(32 + 16) * (size_t)rows * sizeof(float) + 255) & ~(size_t)255;
  const size_t ufb = (untrav_bytes + 255) & ~(size_t)255;
  const size_t pcb = qb;
  const size_t ffb = (face_bytes + 255) & ~(size_t)255;
  x.total = guard + 13 * lb + ub + fb + qb + 256 + ufb + pcb + ffb + guard;
  const size_t b = guard;
  for (int k = 0; k < 13; ++k) x.layer[k] = b + (size_t)k * lb;
  x.untrav = b + 13 * lb;
  x.block_flags = b + 13 * lb + ub;
  x.fp_blocked = b + 13 * lb + ub + fb;
  x.fp_blocked_count = b + 13 * lb + ub + fb + qb;
  x.untrav_flags = b + 13 * lb + ub + fb + qb + 256;
  x.fp_scratch = b + 13 * lb + ub + fb + qb + 256 + ufb;
  x.face_flags = b + 13 * lb + ub + fb + qb + 256 + ufb + pcb;
  x.back_guard = b + 13 * lb + ub + fb + qb + 256 + ufb + pcb + ffb;
  x.first_memset_bytes = guard + 13 * lb + ub + fb;
  x.lb = lb, x.ub = ub, x.fb = fb, x.qb = qb, x.ufb = ufb, x.ffb = ffb, x.guard = guard, x.list_cap = list_cap;
  return x;
}

// one flag per 64 x 16 tile (what fast::normals_fast_max_blocks counts, before its rounding to whole groups)
size_t flag_tiles(int rows, int cols, int batch) { return (size_t)((rows + 63) / 64) * (size_t)((cols + 15) / 16) * (size_t)batch; }
// Layers::untrav_flags: one byte per 64 x 4 cells
size_t untrav_flag_bytes(int rows, int cols, int batch) { return (size_t)((rows + 63) / 64) * (size_t)((cols + 3) / 4) * (size_t)batch; }

void check_shape(int rows, int cols, int batch, size_t fix_flag_count, size_t list_slack) {
  const size_t ufl = untrav_flag_bytes(rows, cols, batch), ffl = te::face_flag_bytes(rows, cols, batch);
  const te::SlabPlan p = te::plan_slab(rows, cols, batch, fix_flag_count, list_slack, ufl, ffl);
  const Expected x = expected(rows, cols, batch, fix_flag_count, list_slack, ufl, ffl);
  const size_t elems = (size_t)rows * cols * batch;
  const te::SlabPart* parts[10] = {&p.front_guard, &p.layers,       &p.mask,        &p.fix_flags,  &p.list,
                                   &p.list_count,  &p.untrav_flags, &p.sum_scratch, &p.face_flags, &p.back_guard};
  const char* names[10] = {"front guard", "layers", "mask", "fix-up flags", "list", "list counter", "untraversable flags", "sum scratch", "face flags", "back guard"};
  // alignment, order, contiguity, total
  CHECK(p.front_guard.off == 0, "%dx%dx%d", rows, cols, batch);
  for (int k = 0; k < 10; ++k) {
    CHECK(parts[k]->off % 256 == 0, "%dx%dx%d: %s at %zu", rows, cols, batch, names[k], parts[k]->off);
    CHECK(parts[k]->bytes > 0, "%dx%dx%d: %s is empty", rows, cols, batch, names[k]);
    if (k > 0) CHECK(parts[k]->off == parts[k - 1]->off + parts[k - 1]->bytes, "%dx%dx%d: %s does not follow %s", rows, cols, batch, names[k], names[k - 1]);
  }
  CHECK(p.total == p.back_guard.off + p.back_guard.bytes, "%dx%dx%d", rows, cols, batch);
  for (int k = 0; k < te::kSlabFloatLayers; ++k) {
    CHECK(p.layer_off(k) % 256 == 0, "%dx%dx%d: layer %d", rows, cols, batch, k);
    CHECK(p.layer_off(k) + elems * sizeof(float) <= p.layers.off + p.layers.bytes, "%dx%dx%d: layer %d", rows, cols, batch, k);
    if (k > 0) CHECK(p.layer_off(k) >= p.layer_off(k - 1) + elems * sizeof(float), "%dx%dx%d: layer %d overlaps", rows, cols, batch, k);
  }
  // every part holds what it is for
  CHECK(p.mask.bytes >= elems, "%dx%dx%d", rows, cols, batch);
  CHECK(p.fix_flags.bytes >= fix_flag_count * sizeof(int), "%dx%dx%d", rows, cols, batch);
  CHECK(p.list_cap == elems + list_slack && p.list.bytes >= p.list_cap * sizeof(unsigned) && p.sum_scratch.bytes == p.list.bytes, "%dx%dx%d", rows, cols, batch);
  CHECK(p.list_count.bytes == 256, "%dx%dx%d", rows, cols, batch);
  CHECK(p.untrav_flags.bytes >= ufl && p.face_flags.bytes >= ffl, "%dx%dx%d", rows, cols, batch);
  // the slack the marches rely on
  const size_t slack = (size_t)te::kSlabGuardRows * (size_t)rows * sizeof(float);
  CHECK(p.layer_off(0) >= slack, "%dx%dx%d: %zu bytes before the first layer, %zu needed", rows, cols, batch, p.layer_off(0), slack);
  CHECK(p.total - (p.face_flags.off + p.face_flags.bytes) >= slack, "%dx%dx%d: slack behind the last part", rows, cols, batch);
  CHECK(p.front_guard.bytes >= slack && p.back_guard.bytes >= slack, "%dx%dx%d", rows, cols, batch);
  // byte for byte the layout te_set_geometry summed by hand
  CHECK(p.total == x.total, "%dx%dx%d: total %zu, expected %zu", rows, cols, batch, p.total, x.total);
  for (int k = 0; k < 13; ++k) CHECK(p.layer_off(k) == x.layer[k], "%dx%dx%d: layer %d", rows, cols, batch, k);
  CHECK(te::kSlabFloatLayers == 13 && p.layer_bytes == x.lb && p.layers.bytes == 13 * x.lb, "%dx%dx%d", rows, cols, batch);
  CHECK(p.mask.off == x.untrav && p.mask.bytes == x.ub, "%dx%dx%d", rows, cols, batch);
  CHECK(p.fix_flags.off == x.block_flags && p.fix_flags.bytes == x.fb, "%dx%dx%d", rows, cols, batch);
  CHECK(p.list.off == x.fp_blocked && p.list.bytes == x.qb && p.list_cap == x.list_cap, "%dx%dx%d", rows, cols, batch);
  CHECK(p.list.off == x.first_memset_bytes, "%dx%dx%d: the first memset range", rows, cols, batch);
  CHECK(p.list_count.off == x.fp_blocked_count, "%dx%dx%d", rows, cols, batch);
  CHECK(p.untrav_flags.off == x.untrav_flags && p.untrav_flags.bytes == x.ufb, "%dx%dx%d", rows, cols, batch);
  CHECK(p.sum_scratch.off == x.fp_scratch && p.sum_scratch.bytes == x.qb, "%dx%dx%d", rows, cols, batch);
  CHECK(p.face_flags.off == x.face_flags && p.face_flags.bytes == x.ffb, "%dx%dx%d", rows, cols, batch);
  CHECK(p.back_guard.off == x.back_guard && p.back_guard.bytes == x.guard && p.front_guard.bytes == x.guard, "%dx%dx%d", rows, cols, batch);
}

// the inputs of the size the shim passes: whole groups of flag tiles, the footprint pass's slack on a device of `cus` units
void check_as_the_shim(int rows, int cols, int batch, int cus) {
  const size_t tiles = flag_tiles(rows, cols, batch);
  check_shape(rows, cols, batch, (tiles + 63) / 64 * 64, te::fast::fp_list_slack(rows, cols, batch, cus));
}

uint64_t g_rng = 1;
uint64_t rnd() {  // splitmix64
  uint64_t z = (g_rng += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

}  // namespace

int main(int argc, char** argv) {
  const int n_random = argc > 1 ? atoi(argv[1]) : 4000;
  g_rng = argc > 2 ? (uint64_t)atoll(argv[2]) : 1;
  const int named[][3] = {{1, 1, 1},       {100, 133, 1},       {63, 17, 3},           {64, 16, 1},
                          {65, 17, 1},     {4096, 4096, 1},     {32768, 32768, 1},     {512, 512, 4200}};
  int n = 0;
  for (const auto& s : named) {
    check_as_the_shim(s[0], s[1], s[2], 256);
    check_as_the_shim(s[0], s[1], s[2], 8);
    n += 2;
  }
  for (int k = 0; k < n_random; ++k, ++n) {
    // small, medium and very large shapes alike; the cell count stays below 2^34 (a slab of 1 TiB)
    const int scale = (int)(rnd() % 3);
    const int lim = scale == 0 ? 130 : (scale == 1 ? 5000 : 70000);
    int rows = 1 + (int)(rnd() % lim), cols = 1 + (int)(rnd() % lim), batch = 1 + (int)(rnd() % (scale == 0 ? 300 : 4));
    while ((double)rows * cols * batch > 17179869184.0) cols = cols / 2 + 1;
    if (k % 2 == 0)
      check_as_the_shim(rows, cols, batch, 1 + (int)(rnd() % 512));
    else
      check_shape(rows, cols, batch, 1 + (size_t)(rnd() % 100000), (size_t)(rnd() % 50000000));
  }
  printf("%d shapes, %d failed checks\n", n, g_failed);
  return g_failed ? 1 : 0;
}
