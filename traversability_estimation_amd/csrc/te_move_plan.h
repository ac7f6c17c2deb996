// te_move_plan.h -- te_move_map as a plan: plain C++, no HIP, shared with the CPU test (tests/cpu/move_plan_check.cpp).
// The index shift of GridMap::move, the rectangles the caller refreshes afterwards, whether the results computed at the old
// position still stand, and the launch geometry of the kernels of te_move.hip.  te_move_geometry hands the public part out as
// it is; te_move_map (te_move.hip) launches by it and decides nothing of its own.
//
// grid_map_core is not in the reference tree, so GridMap::move's arithmetic is RESTATED here from memory, per
// axis, in IEEE double:
//   s = (requested - held) / resolution;  shift = (int)(s + 0.5 * sign(s));  new position = held + shift * resolution.
// Buffer order: x(i) = ax - res * i (te_geom.h: cell_x), so a map moved by +k cells in x holds its old cell i at i + k.
// A zero shift on both axes returns early: nothing changes, not even the position.
//
// Results kept: the reference decides a cell exactly on a disc's circle from the rounded double positions of the cells, centre
// by centre (te_disc.h: the tie offsets), so a result computed at the old position can differ on such a cell from one computed at
// the new position.  With a tie disc among the five of the parameters nothing computed is kept.  The predicate is the
// classification that routes the kernels -- build_disc_table (te_disc_table.h), which is build_disc's and build_fp_table's
// (the same q and the same tolerance) without their size bounds; a radius that is not a positive finite number counts as a tie.
#pragma once
#include <math.h>
#include <stddef.h>

#include "te_disc_table.h"
#include "travgpu.h"

namespace te {
namespace move {

constexpr int kLanes = 64;  // threads along a column: one group of four cells each
constexpr int kCols = 4;    // columns of a workgroup
constexpr unsigned kMaxGridX = 1024, kMaxGridY = 4096;  // (grid-stride beyond, both ways)
constexpr double kMaxShift = 1073741824.0;               // 2^30 cells: the clamp of |s| before the cast

// GridMap::move's shift of one axis
inline int axis_shift(double held, double requested, double res) {
  double s = (requested - held) / res;
  if (s > kMaxShift) s = kMaxShift;
  if (s < -kMaxShift) s = -kMaxShift;
  const double sign = s > 0.0 ? 1.0 : (s < 0.0 ? -1.0 : 0.0);
  return (int)(s + 0.5 * sign);
}

// a disc of the parameters has cells on its circle (or cannot be classified)
inline bool tie_disc(double radius, double res) {
  if (!(radius > 0.0) || !isfinite(radius) || !(radius / res < 1e6)) return true;  // (the table is O(radius / res) ints)
  DiscTable t;
  build_disc_table(radius, res, &t);
  return t.n_ties() != 0;
}
// the five discs: normals, roughness, both step windows, footprint radius + offset
inline bool any_tie_disc(const te_params& p, double res) {
  return tie_disc(p.normals_radius, res) || tie_disc(p.rough_radius, res) || tie_disc(p.step_radius1, res) || tie_disc(p.step_radius2, res) ||
         tie_disc(p.fp_radius + p.fp_offset, res);
}

struct Plan {
  te_move_info info;
  // new cell (i, j) takes old cell (i - shift_rows, j - shift_cols); the new rows [i_lo, i_hi) and columns [j_lo, j_hi) have
  // a source (empty ranges when all_exposed)
  int i_lo, i_hi, j_lo, j_hi;
  size_t scratch_bytes;     // one float layer of one map; 0: no kernel runs (zero shift, all exposed)
  unsigned grid_x, grid_y;  // k_move_shift over one layer of one map, block (kLanes, kCols)
};

// TE_ERR_INVALID_ARG / TE_ERR_BAD_PARAM (and *why, a literal) as include/travgpu.h states them; `raster`: TE_OPT_NORMALS_ALGORITHM = 1
inline int plan(int rows, int cols, double res, double pos_x, double pos_y, double new_x, double new_y, const te_params* params, bool raster,
                Plan* out, const char** why) {
  *out = Plan();
  te_move_info& m = out->info;
  if (rows <= 0 || cols <= 0 || !(res > 0.0) || !isfinite(res) || !isfinite(pos_x) || !isfinite(pos_y)) {
    *why = "bad map geometry";
    return TE_ERR_INVALID_ARG;
  }
  if (!isfinite(new_x) || !isfinite(new_y)) {
    *why = "the requested position is not finite";
    return TE_ERR_BAD_PARAM;
  }
  const int kr = axis_shift(pos_x, new_x, res), kc = axis_shift(pos_y, new_y, res);
  m.pos_x = pos_x;
  m.pos_y = pos_y;
  m.results_kept = 1;
  if (kr == 0 && kc == 0) return TE_OK;  // (upstream returns early: the position stays bit for bit)
  m.shift_rows = kr;
  m.shift_cols = kc;
  m.pos_x = pos_x + (double)kr * res;
  m.pos_y = pos_y + (double)kc * res;
  m.results_kept = (params && !raster && !any_tie_disc(*params, res)) ? 1 : 0;
  auto rect = [&m](int row0, int col0, int h, int w, int exposed) {
    int* r = m.rects[m.n_rects];
    r[0] = row0, r[1] = col0, r[2] = h, r[3] = w;
    m.rect_exposed[m.n_rects++] = exposed;
  };
  const long long ar = kr < 0 ? -(long long)kr : kr, ac = kc < 0 ? -(long long)kc : kc;
  if (ar >= rows || ac >= cols) {
    m.all_exposed = 1;
    rect(0, 0, rows, cols, 1);
    return TE_OK;
  }
  out->i_lo = kr > 0 ? kr : 0;
  out->i_hi = kr < 0 ? rows + kr : rows;
  out->j_lo = kc > 0 ? kc : 0;
  out->j_hi = kc < 0 ? cols + kc : cols;
  // exposed: the band of rows over the full width, then the band of columns over the rows that are left
  if (kr != 0) rect(kr > 0 ? 0 : out->i_hi, 0, (int)ar, cols, 1);
  if (kc != 0) rect(out->i_lo, kc > 0 ? 0 : out->j_hi, out->i_hi - out->i_lo, (int)ac, 1);
  // trailing lines: the border opposite to the exposed band of each axis that moved
  if (kr != 0) rect(kr > 0 ? rows - 1 : 0, 0, 1, cols, 0);
  if (kc != 0) rect(0, kc > 0 ? cols - 1 : 0, rows, 1, 0);
  out->scratch_bytes = (size_t)rows * (size_t)cols * sizeof(float);
  const long long slots = (long long)(rows >> 2) + 2, bx = (slots + kLanes - 1) / kLanes, by = ((long long)cols + kCols - 1) / kCols;
  out->grid_x = bx > kMaxGridX ? kMaxGridX : (unsigned)bx;
  out->grid_y = by > kMaxGridY ? kMaxGridY : (unsigned)by;
  return TE_OK;
}

}  // namespace move
}  // namespace te
