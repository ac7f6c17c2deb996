// te_fp_route.h -- which kernels sum the circular footprint pass, decided once per launch on the host.
// Plain C++ of plain values: launch_footprint (te_footprint.hip) routes with plan_fp_route and hands the result to the
// launcher of the route, which decides nothing; the CPU check (tests/cpu/fp_route_check.cpp, tests/test_fp_route.py) runs
// the same code on DESIGN.md's cases and on a sweep, and holds it to what the kernels rely on.
#pragma once
#include <math.h>
#include <stddef.h>

#include "te_strips.h"
#include "te_tie_triple.h"

// The shapes the kernel parts instantiate (Q: the disc's largest di^2 + dj^2, te_march.h).  k_fp_slide3: every disc shape
// up to radius 10 except the single cell, and for radii 11 .. 16 every sum of two squares up to 256; k_fp_slide5: the
// same below 256 (2R+1 <= 31).  Each list is compiled in five parts (build.py); part k instantiates TE_F3_Pk / TE_F5_Pk.
#define TE_F3_P0(X) X(4) X(16) X(26) X(37) X(50) X(65) X(73) X(85) X(100) X(121) X(136) X(148) X(162) X(178) X(193) X(202) X(212) X(229) X(256)
#define TE_F3_P1(X) X(10) X(13) X(25) X(36) X(49) X(64) X(82) X(98) X(109) X(117) X(130) X(146) X(160) X(173) X(185) X(200) X(226) X(241) X(250)
#define TE_F3_P2(X) X(9) X(20) X(34) X(45) X(58) X(61) X(81) X(97) X(106) X(116) X(128) X(145) X(157) X(170) X(181) X(197) X(225) X(234) X(245)
#define TE_F3_P3(X) X(2) X(8) X(18) X(32) X(41) X(53) X(72) X(80) X(90) X(104) X(113) X(125) X(144) X(153) X(169) X(196) X(208) X(221) X(233) X(244)
#define TE_F3_P4(X) X(1) X(5) X(17) X(29) X(40) X(52) X(68) X(74) X(89) X(101) X(122) X(137) X(149) X(164) X(180) X(194) X(205) X(218) X(232) X(242)
#define TE_F5_P0(X) X(4) X(16) X(26) X(37) X(50) X(65) X(73) X(85) X(100) X(121) X(136) X(148) X(162) X(178) X(193) X(202) X(212) X(229)
#define TE_F5_P1(X) X(10) X(13) X(25) X(36) X(49) X(64) X(82) X(98) X(109) X(117) X(130) X(146) X(160) X(173) X(185) X(200) X(226) X(241) X(250)
#define TE_F5_P2(X) X(9) X(20) X(34) X(45) X(58) X(61) X(81) X(97) X(106) X(116) X(128) X(145) X(157) X(170) X(181) X(197) X(225) X(234) X(245)
#define TE_F5_P3(X) X(2) X(8) X(18) X(32) X(41) X(53) X(72) X(80) X(90) X(104) X(113) X(125) X(144) X(153) X(169) X(196) X(208) X(221) X(233) X(244)
#define TE_F5_P4(X) X(1) X(5) X(17) X(29) X(40) X(52) X(68) X(74) X(89) X(101) X(122) X(137) X(149) X(164) X(180) X(194) X(205) X(218) X(232) X(242)
// k_fp_slide4<Q, true>: the whole-cell radii 1 .. 16 (Q = R^2)
#define TE_F4_SHAPES_ALL(X) X(1) X(4) X(9) X(16) X(25) X(36) X(49) X(64) X(81) X(100) X(121) X(144) X(169) X(196) X(225) X(256)

namespace te {
namespace fast {

// The double kernels (k_fp_slide3, k_fp_slide<R>) store one double per cell, T' + kFpUOff * U (T': the traversability value or
// the default, U: 1 for an untraversable cell), sum it over the disc and split the sum again: the count of untraversable
// cells is floor((S + kFpUOff / 2) / kFpUOff), a single cell is untraversable when its value reaches kFpUOff / 2.  Exact,
// and right, while every |T'| and every disc's |sum T'| stay below kFpUOff / 2 -- which only a bound on the layer can
// promise (fp_packed_ok); without one the pass takes the route of any reach, which counts U in integers.
constexpr double kFpUOff = 4096.0;
constexpr int kF5Waves = 5;                 // waves per SIMD k_fp_slide5 is compiled for
constexpr int kF5UBit = 27;                 // k_fp_slide5's untraversable flag: a disc's fixed-point T-sum stays below it
constexpr int kF4Waves = 4;                 // waves per SIMD k_fp_slide4 is compiled for
constexpr int kF4Chunk = 256;               // entries of the list a block reserves at a time
constexpr unsigned kF4NoCell = 0xffffffffu;  // an unused entry

#define TE_FP_CASE(q) case q:
inline bool fp_f3_shape(int q) { switch (q) { TE_F3_P0(TE_FP_CASE) TE_F3_P1(TE_FP_CASE) TE_F3_P2(TE_FP_CASE) TE_F3_P3(TE_FP_CASE) TE_F3_P4(TE_FP_CASE) return true; default: return false; } }
inline bool fp_f5_shape(int q) { switch (q) { TE_F5_P0(TE_FP_CASE) TE_F5_P1(TE_FP_CASE) TE_F5_P2(TE_FP_CASE) TE_F5_P3(TE_FP_CASE) TE_F5_P4(TE_FP_CASE) return true; default: return false; } }
inline bool fp_f4_shape(int q) { switch (q) { TE_F4_SHAPES_ALL(TE_FP_CASE) return true; default: return false; } }
#undef TE_FP_CASE

// The fixed-point exponent of k_fp_slide4 / k_fp_slide5: the largest k <= 23 such that `cells` values of at most
// cap * 2^k + 1/2 each stay below `limit` (-1: none)
inline int fp_fixed_k(double cells, double cap, double limit) {
  int k = 23;
  while (k >= 0 && cells * (cap * ldexp(1.0, k) + 1.0) >= limit) --k;
  return k;
}

// The bound the double kernels need: `cells` values (the whole disc, the cells on its circle included) of magnitude at most
// max(tcap, |def|) sum to less than kFpUOff / 2.  tcap: the bound of the finite values of a layer the chain wrote with
// non-negative weights (they lie in [0, tcap]), < 0: none known; def: the value that replaces NaN, of either sign.
inline bool fp_packed_ok(double cells, double tcap, double def) {
  if (!(tcap >= 0.0) || !(fabs(def) <= 1.7976931348623157e308)) return false;
  const double cap = (tcap > fabs(def) ? tcap : fabs(def)) * (1.0 + 1e-6) + 1e-12;
  return cells * cap < 0.5 * kFpUOff;
}

// Entries of the list beyond one per cell: every block of k_fp_slide4 may leave one chunk unfinished, and a launch has
// at most (resident blocks + one row of blocks) of them -- or, when the strips are clamped to 512 rows (a very tall
// map, a small device), one block per 512 rows of every block column (the route checks the actual grid against it).
inline size_t fp_list_slack(int rows, int cols, int batch, int cus) {
  const size_t nbx = (size_t)(rows + 63) / 64, nb = (size_t)(batch > 0 ? batch : 1);
  const size_t one_round = (size_t)32 * (size_t)cus + 2 * nbx * nb;  // (up to 8 waves per SIMD: k_fp_slide5 runs at 5)
  const size_t clamped = nbx * nb * ((size_t)(cols + 511) / 512 + 1);
  // k_fp_slide5 reserves 64 entries per row of EVERY block column, the shifted last one included: a map whose rows are
  // not a multiple of 64 needs the columns that block shares with its neighbour once more -- without them rows = 65 or
  // 4033 failed the route's capacity test and fell to the double kernel for no other reason
  const size_t shared = (nbx * 64 - (size_t)rows) * (size_t)cols * nb;
  return (size_t)kF4Chunk * (one_round > clamped ? one_round : clamped) + shared;
}

enum FpRouteKind { kFpSlide5, kFpSlide4, kFpSlide3, kFpGeneral, kFpAny };

struct FpRouteIn {
  // the footprint disc (build_disc and tie_summary of te_disc.h) and its spiral
  int R, Q, npoints, n_ties;
  bool ties_on_circle;  // every tie offset has the squared norm reach^2 (a whole-cell radius)
  int n_gen;            // tie offsets with both parts non-zero
  int reach, n_spiral;
  double rmin, def;
  double tcap;  // upper bound of the finite values of the traversability layer (written by the chain), < 0: none known
  // the maps, and the cells the pass covers: the (non-empty) region [i0, i1) x [j0, j1) of one map, or (region false) all of them
  int rows, cols, batch;
  bool region;
  int i0, i1, j0, j1;
  // the buffers of the context
  bool guard_rows;  // the traversability layer and the mask have the slab's guard rows (layer_has_guard_rows)
  bool has_list, has_scratch;  // Layers::fp_blocked + fp_blocked_count, Layers::fp_scratch
  size_t list_cap;             // Layers::fp_blocked_cap
  int cus;                     // compute units of the device
  bool any;                    // FootprintParams::any: the route of any reach (asked for, or a reach above 20 cells)
  // measurement switches of the lab build (TE_NO_F3 / F4 / F5, TE_F4_NO_TIES, TE_F5_WAVES, TE_F5_MAX_STRIP,
  // TE_F4_BLOCKS_PER_CU, TE_F4_MIN_STRIP); the defaults are the shipped library's
  bool no_f3 = false, no_f4 = false, no_f5 = false, f4_no_ties = false;
  int f5_waves = 0, f5_max_strip = 512, f4_blocks_per_cu = 0, f4_min_strip = 1;
};

struct FpRoute {
  FpRouteKind route = kFpGeneral;
  int k = -1;          // fixed-point exponent (slide4, slide5)
  int strip_rows = 0;  // rows per strip and list chunk (slide4, slide5)
  int chunk = 0;
  bool blocked = false;  // k_fp_blocked follows (the listed discs)
};

inline FpRoute plan_fp_route(const FpRouteIn& in) {
  if (in.any) return FpRoute{kFpAny};
  const int nbx_l = in.region ? (in.i1 - 1) / 64 - in.i0 / 64 + 1 : (in.rows + 63) / 64;
  const int H = in.region ? in.j1 - in.j0 : in.cols;
  const int nz = in.region ? 1 : (in.batch > 0 ? in.batch : 1);
  const double cells = (double)in.rows * (double)in.cols;
  // the shape-specialised kernels: a map at least one wavefront and one disc wide, 32-bit byte offsets within a pass
  auto map_ok = [&](int R) { return in.rows >= 64 && in.rows >= 2 * R + 1 && in.cols >= 2 * R + 1 && cells * 4.0 < 4294967296.0; };
  // the fixed-point kernels: one list entry per cell, and a bound on the values (the default that replaces NaN included)
  const bool list_ok = in.has_list && cells * (double)in.batch <= (double)in.list_cap;
  const bool bounded = in.tcap >= 0.0 && in.def >= 0.0;
  const double cap = (in.tcap > in.def ? in.tcap : in.def) * (1.0 + 1e-6) + 1e-12;
  const bool tie_free = in.n_ties == 0 && in.Q >= 1 && in.R >= 1 && in.reach == in.R && map_ok(in.R);
  // k_fp_slide5: tie-free, 2R+1 <= 31 (a run sum of 2R+1 cells below the flag bit); rounding each value to 2^-k with
  // k < 17 could show at the 1e-5 level
  if (!in.no_f5 && tie_free && 2 * in.R + 1 <= 31 && fp_f5_shape(in.Q) && list_ok && in.has_scratch && bounded && in.guard_rows) {
    const int k = fp_fixed_k((double)in.npoints, cap, (double)(1u << kF5UBit));
    if (k >= 17) {
      const int capacity = (in.f5_waves > 0 ? in.f5_waves : kF5Waves) * 4 * in.cus;
      const int sr = plan_strip_rows(H, (long)nbx_l * nz, capacity, in.f5_max_strip > 0 ? in.f5_max_strip : 512);
      const int chunk = sr >= 4 ? kF4Chunk : (sr * 64 >= kF4Chunk / 2 ? kF4Chunk / 2 : 64);  // (a strip of one row lists at most 64 cells)
      const int nstrips = (H + sr - 1) / sr;
      // a block reserves at most its own cells rounded up to whole chunks (64 entries per row of every block column -- a
      // shifted last block reserves for the columns it shares with its neighbour too)
      // (radiusMin = 0: the march writes the blocked discs' 0 itself, no k_fp_blocked)
      if ((double)nbx_l * (double)nz * ((double)H * 64.0 + (double)nstrips * (double)chunk) <= (double)in.list_cap)
        return FpRoute{kFpSlide5, k, sr, chunk, in.rmin != 0.0};
    }
  }
  // k_fp_slide4<R^2, true>: a whole-cell tie radius (the kernel knows the circle's cells from R: the axis cells and one
  // Pythagorean triple); the packed edge sums of 2R+1 cells stay below 2^24
  const int R4 = in.reach;
  if (!in.no_f4 && !in.f4_no_ties && in.n_ties != 0 && in.ties_on_circle && R4 >= 1 && map_ok(R4) && fp_f4_shape(R4 * R4) &&
      in.n_gen == tie_triple_cells(R4) && in.n_ties == 4 + in.n_gen && list_ok && bounded) {
    const int k = fp_fixed_k((double)(2 * R4 + 1), cap, 16777216.0);
    if (k >= 17) {
      const int lds = (2 * R4 + 2) * (64 + 2 * R4) * 4;
      int per_cu = (160 * 1024) / (((lds + 2047) / 2048) * 2048);  // see te_normals3.hip (resident_blocks)
      if (per_cu > kF4Waves * 4) per_cu = kF4Waves * 4;
      if (in.f4_blocks_per_cu > 0 && in.f4_blocks_per_cu < kF4Waves * 4) per_cu = in.f4_blocks_per_cu;
      int strips = per_cu * in.cus / (nbx_l * nz > 0 ? nbx_l * nz : 1);
      strips = strips < 1 ? 1 : strips;
      int sr = (H + strips - 1) / strips;
      // small maps cannot fill the wave slots: every resident block runs at once, so the launch takes one warm-up plus
      // the rows of one strip -- the shortest strips win (the spiral walks of a row are serial within its wavefront)
      sr = sr < in.f4_min_strip ? in.f4_min_strip : (sr > 512 ? 512 : sr);
      sr = sr < 1 ? 1 : sr;
      const int chunk = sr >= 4 ? kF4Chunk : (sr * 64 >= kF4Chunk / 2 ? kF4Chunk / 2 : 64);
      const int nstrips = (H + sr - 1) / sr;
      // every listed cell takes one entry and every block may leave one chunk unfinished (closed chunks are full)
      if ((double)nbx_l * (double)nstrips * (double)nz * (double)chunk + cells * (double)nz <= (double)in.list_cap)
        return FpRoute{kFpSlide4, k, sr, chunk, in.rmin != 0.0};
    }
  }
  // The double kernels pack the untraversable count into the sum (kFpUOff): only under a bound that keeps the two apart.
  // Every other layer -- uploaded, written by an expression or through te_device_ptr, combined with a negative or a large
  // weight, a large default -- takes the route of any reach, whose count is an integer of its own.
  if (!fp_packed_ok((double)in.npoints + (double)in.n_ties, in.tcap, in.def)) return FpRoute{kFpAny};
  // k_fp_slide3<Q> (double): tie-free, the spiral within the kernel's table registers
  if (!in.no_f3 && tie_free && fp_f3_shape(in.Q) && in.n_spiral <= ((int)(3.2 * (in.R + 1) * (in.R + 1) / 64) + 1) * 64)
    return FpRoute{kFpSlide3};
  return FpRoute{kFpGeneral};  // k_fp_slide<R>: any reach up to 20 cells, always the region's whole map
}

}  // namespace fast
}  // namespace te
