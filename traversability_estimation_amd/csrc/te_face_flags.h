// te_face_flags.h -- "this part of the map holds no vertical face": one byte per 64 x 4 cells of every map, built from the
// elevation alone by the upload's pass over the layer (k_count_invalid, te_shim.hip) and read by the mask kernel of the
// footprint pass (k_fp_mask, te_footprint.hip), which skips the whole step-check staging on tiles whose bytes are all clear.
//
// k_fp_mask decides per tile whether any cell has a lower step neighbour (tile_has_kl):
//     hit(n)  = (double)min3x3(t_key)(n) < (double)elev(n) - crit_step        t_key = elevation where step == 0, NaN elsewhere
// with a NaN-ignoring minimum.  The same expression on the plain elevation,
//     hit'(n) = (double)min3x3(elev)(n)  < (double)elev(n) - crit_step,
// is a superset cell by cell: min3x3(elev) <= min3x3(t_key) whenever the latter is a number, and a NaN minimum compares
// false.  hit' does not depend on the step scores, so it can be evaluated once per uploaded elevation.
//
// A flag is 1 iff some in-map cell within Chebyshev distance kFaceDilate of its granule has hit' (cells outside the map count
// as NaN): kFaceDilate = 2 is how far beyond its own cells a mask tile evaluates `hit`, so a tile without any `hit` cell is
// one whose own flags -- MY / 4 bytes of one flag column -- are all clear, whatever the tile height MY.
// The flags are valid for the crit_step (te_params::fp_critical_step) they were built with.
//
// Plain C++ for host and device: the kernels, the launch code and the CPU test (tests/cpu/face_flags_check.cpp) compile
// the same geometry and the same predicate.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TE_FF_HD __host__ __device__ __forceinline__
#else
#define TE_FF_HD inline
#endif

namespace te {

constexpr int kFaceGranI = 64, kFaceGranJ = 4;  // cells of a granule along i (the fast axis) and j: the layout of Layers::untrav_flags
constexpr int kFaceDilate = 2;                  // k_fp_mask computes t_kl this far beyond a tile's own cells (MH - 1)

TE_FF_HD int face_flag_ntx(int rows) { return (rows + kFaceGranI - 1) / kFaceGranI; }
TE_FF_HD int face_flag_nfy(int cols) { return (cols + kFaceGranJ - 1) / kFaceGranJ; }
TE_FF_HD size_t face_flag_bytes(int rows, int cols, int batch) {
  return (size_t)face_flag_ntx(rows) * (size_t)face_flag_nfy(cols) * (size_t)batch;
}
// the byte of the granule that holds cell (i, j) of map `map`
TE_FF_HD size_t face_flag_index(int rows, int cols, int map, int i, int j) {
  return ((size_t)map * (size_t)face_flag_nfy(cols) + (size_t)(j / kFaceGranJ)) * (size_t)face_flag_ntx(rows) + (size_t)(i / kFaceGranI);
}

// NaN-ignoring minimum (NaN only if both are)
TE_FF_HD float face_min(float a, float b) { return (b < a || a != a) ? b : a; }
// the mask kernel's own test (:825 of the reference in its double arithmetic) of a cell of elevation e against the 3x3 minimum m
TE_FF_HD bool face_hit(float m, float e, double crit_step) { return (double)m < (double)e - crit_step; }

// Does the tile of cells [i0, i0 + tw) x [j0, j0 + th) hold a cell within 3 cells of a border side on which the 2.5 res submap
// lookup fails (edge_fail: bit 0 i == 0, bit 1 i == rows - 1, bit 2 j == 0, bit 3 j == cols - 1)?  Those cells' step
// checks are decided by the full checkForStep on the staged tiles whatever the screen says: such a tile is never flat.
TE_FF_HD bool face_tile_near_failing_border(int rows, int cols, int edge_fail, int i0, int j0, int tw, int th) {
  return ((edge_fail & 1) && i0 <= 2) || ((edge_fail & 2) && i0 + tw - 1 >= rows - 3) || ((edge_fail & 4) && j0 <= 2) ||
         ((edge_fail & 8) && j0 + th - 1 >= cols - 3);
}

// Are the flags of the tile [i0, i0 + 64) x [j0, j0 + th) of map `map` all clear?  (i0 a multiple of 64, j0 and th of 4.)
TE_FF_HD bool face_tile_clear(const uint8_t* flags, int rows, int cols, int map, int i0, int j0, int th) {
  const int ntx = face_flag_ntx(rows), nfy = face_flag_nfy(cols);
  const uint8_t* f = flags + ((size_t)map * (size_t)nfy) * (size_t)ntx + (size_t)(i0 / kFaceGranI);
  unsigned any = 0;
  for (int t = 0; t < th / kFaceGranJ; ++t) {
    const int fj = j0 / kFaceGranJ + t;
    if (fj < nfy) any |= f[(size_t)fj * (size_t)ntx];
  }
  return any == 0;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The definition, cell by cell on the host (column-major maps: cell (i, j) of map m at m * rows * cols + j * rows + i):
// what k_count_invalid must leave in `flags` (face_flag_bytes() bytes).  `hit` (rows * cols * batch bytes, or nullptr)
// receives hit' per cell.
inline void face_flags_host(const float* elev, int rows, int cols, int batch, double crit_step, uint8_t* flags, uint8_t* hit = nullptr) {
  const size_t nflags = face_flag_bytes(rows, cols, batch);
  for (size_t k = 0; k < nflags; ++k) flags[k] = 0;
  const float nan = __builtin_nanf("");
  for (int m = 0; m < batch; ++m) {
    const float* e = elev + (size_t)m * rows * cols;
    for (int j = 0; j < cols; ++j)
      for (int i = 0; i < rows; ++i) {
        float mn = nan;
        for (int dj = -1; dj <= 1; ++dj)
          for (int di = -1; di <= 1; ++di) {
            const int a = i + di, b = j + dj;
            if (a >= 0 && a < rows && b >= 0 && b < cols) mn = face_min(mn, e[(size_t)b * rows + a]);
          }
        const bool h = face_hit(mn, e[(size_t)j * rows + i], crit_step);
        if (hit) hit[(size_t)m * rows * cols + (size_t)j * rows + i] = h ? 1 : 0;
        if (!h) continue;
        // every granule within kFaceDilate cells of (i, j)
        const int a0 = i - kFaceDilate < 0 ? 0 : i - kFaceDilate, a1 = i + kFaceDilate > rows - 1 ? rows - 1 : i + kFaceDilate;
        const int b0 = j - kFaceDilate < 0 ? 0 : j - kFaceDilate, b1 = j + kFaceDilate > cols - 1 ? cols - 1 : j + kFaceDilate;
        for (int gj = b0 / kFaceGranJ; gj <= b1 / kFaceGranJ; ++gj)
          for (int gi = a0 / kFaceGranI; gi <= a1 / kFaceGranI; ++gi) flags[face_flag_index(rows, cols, m, gi * kFaceGranI, gj * kFaceGranJ)] = 1;
      }
  }
}
#endif

}  // namespace te
