// te_shapes.h -- the disc shapes the shape-specialised filter kernels are instantiated for, and "is this shape instantiated"
// beside every list.  Plain C++ (no HIP): the kernel files instantiate from these macros, plan_chain_route
// (te_chain_route.h) asks the functions, and the CPU check (tests/cpu/chain_route_check.cpp) compiles the same text.
#pragma once

namespace te {
namespace fast {

constexpr int isqrt_c(int v) {
  int r = 0;
  while ((r + 1) * (r + 1) <= v) ++r;
  return r;
}

template <int Q>
struct Shape {
  static constexpr int R = isqrt_c(Q);
  static constexpr int P = 2 * R + 1;  // accumulators in flight == rows per unrolled period
  // half-width of the run at column offset d (0 <= d <= R)
  static constexpr int hw(int d) { return isqrt_c(Q - d * d); }
  static constexpr int npoints() {
    int n = 0;
    for (int d = -R; d <= R; ++d) n += 2 * hw(d < 0 ? -d : d) + 1;
    return n;
  }
};

// The disc shapes (Q = largest di^2+dj^2 in the disc) with radius up to 10 cells: every sum of two squares <= 100.
// The step marches (te_step5.hip) and the shape form of k_normals_slide (te_slide_normals.hip, Q >= 1) exist for each.
#ifndef TE_DISC_SHAPES  // (tools: -D'TE_DISC_SHAPES(X)=X(81)' compiles one shape)
#define TE_DISC_SHAPES(X) \
  X(0) X(1) X(2) X(4) X(5) X(8) X(9) X(10) X(13) X(16) X(17) X(18) X(20) X(25) X(26) X(29) X(32) X(34) X(36) X(37) \
  X(40) X(41) X(45) X(49) X(50) X(52) X(53) X(58) X(61) X(64) X(65) X(68) X(72) X(73) X(74) X(80) X(81) X(82) X(85) \
  X(89) X(90) X(97) X(98) X(100)
#endif
// k_normals3 / k_normals3s (te_normals3.hip): every disc shape except the single cell, compiled in six parts (build.py);
// part k instantiates TE_N3_Pk
#define TE_N3_P0(X) X(9) X(20) X(32) X(52) X(61) X(72) X(100)
#define TE_N3_P1(X) X(8) X(18) X(29) X(50) X(58) X(82) X(98)
#define TE_N3_P2(X) X(5) X(17) X(26) X(49) X(53) X(81) X(97)
#define TE_N3_P3(X) X(4) X(16) X(37) X(45) X(68) X(80) X(90)
#define TE_N3_P4(X) X(10) X(13) X(36) X(41) X(65) X(74) X(89)
#define TE_N3_P5(X) X(1) X(2) X(25) X(34) X(40) X(64) X(73) X(85)
// The RAW step marches: the shapes a whole-cell radius of 3 .. 10 cells leaves without its circle (2 cells: k_step_small)
#define TE_STEP_RAW_SHAPES(X) X(8) X(13) X(20) X(34) X(45) X(61) X(80) X(98)

#define TE_SHAPE_CASE(q) case q:
constexpr bool disc_shape(int q) { switch (q) { TE_DISC_SHAPES(TE_SHAPE_CASE) return true; default: return false; } }
constexpr bool n3_shape(int q) { switch (q) { TE_N3_P0(TE_SHAPE_CASE) TE_N3_P1(TE_SHAPE_CASE) TE_N3_P2(TE_SHAPE_CASE) TE_N3_P3(TE_SHAPE_CASE) TE_N3_P4(TE_SHAPE_CASE) TE_N3_P5(TE_SHAPE_CASE) return true; default: return false; } }
constexpr bool step_raw_shape(int q) { switch (q) { TE_STEP_RAW_SHAPES(TE_SHAPE_CASE) return true; default: return false; } }
#undef TE_SHAPE_CASE
// k_normals_slide<R, -1>: the radius form, for tie-free discs whose shape has no instantiation of its own
constexpr int kSlideMaxRadius = 16;
constexpr bool slide_radius(int R) { return R >= 1 && R <= kSlideMaxRadius; }

}  // namespace fast
}  // namespace te
