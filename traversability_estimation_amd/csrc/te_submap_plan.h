// te_submap_plan.h -- the geometry of a submap request as a plan: plain C++, no HIP, shared with the CPU test
// (tests/cpu/submap_plan_check.cpp).  te_submap_geometry hands it out as it is; te_download_submap(_msg) (te_submap.hip)
// takes the rectangle its kernel packs from it.
//
// The reference answers its get_traversability service with GridMap::getSubmap(position, length)
// (TraversabilityEstimation.cpp:297-316).  grid_map_core is not in the reference tree, so getSubmap / getSubmapInformation are
// RESTATED here for a map whose start index is (0, 0) -- device layers never have another -- in IEEE double, in grid_map's
// order of operations (tests/ref_py/grid_map_ref.py::GridMapRef.submap spells the same order out, independently):
//   1. the requested corners position +- length / 2 are bounded to the map (boundPositionToRange: a corner on or outside a
//      border moves 10 eps -- times |coordinate| above 1 -- inside it);
//   2. the top-left and bottom-right indices are the truncating getIndexFromPosition of the bounded corners; a corner that
//      is still outside the map (checkIfPositionWithinMap) fails the request            -- exits 1 and 2;
//   3. the top-left index must be a cell of the map (getPositionFromIndex)                -- exit 3;
//   4. size = bottom-right - top-left + 1 cells; the submap's length is size * resolution, its position the centre of that
//      rectangle, found from the top-left cell's outer corner;
//   5. the requested centre must lie inside the submap ("requested index in submap")     -- exit 4.
// Exits 3 and 4 are one `return false` each in grid_map and one failure class in GridMapRef.submap; whichever is taken, ok
// is 0 and nothing else of the plan is meaningful.
#pragma once
#include <math.h>

#include "travgpu.h"

namespace te {
namespace submap {

// one axis of a grid map: cells, length = cells * resolution, the map's centre
struct Axis {
  int n;
  double res, len, pos;
};

// boundPositionToRange
inline double bound_to_range(const Axis& a, double p) {
  double shifted = (p - a.pos) + 0.5 * a.len;
  double eps = 10.0 * 2.220446049250313e-16;  // 10 * numeric_limits<double>::epsilon()
  if (fabs(p) > 1.0) eps *= fabs(p);
  if (shifted <= 0.0)
    shifted = eps;
  else if (shifted >= a.len)
    shifted = a.len - eps;
  return (shifted + a.pos) - 0.5 * a.len;
}
// checkIfPositionWithinMap
inline bool inside(const Axis& a, double p) {
  const double t = -((p - a.pos) - 0.5 * a.len);
  return t >= 0.0 && t < a.len;
}
// getIndexFromPosition of a position inside the map (the cast truncates towards zero; inside: the value fits an int)
inline int index_of(const Axis& a, double p) { return (int)(-(((p - 0.5 * a.len) - a.pos) / a.res)); }
// getPositionFromIndex
inline double position_of(const Axis& a, int idx) { return (a.pos + (0.5 * a.len - 0.5 * a.res)) + a.res * (double)(-idx); }

// The plan of one request.  TE_ERR_INVALID_ARG (and *why, a literal) for arguments no map geometry or request can have;
// TE_OK otherwise, with out->ok = 0 for a request getSubmap refuses.
inline int plan(int rows, int cols, double resolution, double pos_x, double pos_y, double req_x, double req_y, double req_len_x,
                double req_len_y, te_submap_info* out, const char** why) {
  *out = te_submap_info();
  if (rows <= 0 || cols <= 0 || !(resolution > 0.0) || !isfinite(resolution) || !isfinite(pos_x) || !isfinite(pos_y)) {
    *why = "bad map geometry";
    return TE_ERR_INVALID_ARG;
  }
  if (!isfinite(req_x) || !isfinite(req_y) || !isfinite(req_len_x) || !isfinite(req_len_y)) {
    *why = "the requested position or length is not finite";
    return TE_ERR_INVALID_ARG;
  }
  if (req_len_x < 0.0 || req_len_y < 0.0) {
    *why = "the requested length is negative";
    return TE_ERR_INVALID_ARG;
  }
  const Axis ax[2] = {{rows, resolution, (double)rows * resolution, pos_x}, {cols, resolution, (double)cols * resolution, pos_y}};
  const double req[2] = {req_x, req_y}, req_len[2] = {req_len_x, req_len_y};
  int tl[2], br[2];
  for (int k = 0; k < 2; ++k) {  // exit 1: the bounded top-left corner (both axes are tested before either index is used)
    const double c = bound_to_range(ax[k], req[k] + 0.5 * req_len[k]);
    if (!inside(ax[k], c)) return TE_OK;
    tl[k] = index_of(ax[k], c);
  }
  for (int k = 0; k < 2; ++k) {  // exit 2: the bounded bottom-right corner
    const double c = bound_to_range(ax[k], req[k] - 0.5 * req_len[k]);
    if (!inside(ax[k], c)) return TE_OK;
    br[k] = index_of(ax[k], c);
  }
  for (int k = 0; k < 2; ++k)  // exit 3
    if (tl[k] < 0 || tl[k] >= ax[k].n) return TE_OK;
  int size[2];
  double sub_len[2], sub_pos[2];
  for (int k = 0; k < 2; ++k) {
    const double corner = position_of(ax[k], tl[k]) + 0.5 * resolution;
    size[k] = br[k] - tl[k] + 1;
    sub_len[k] = (double)size[k] * resolution;
    sub_pos[k] = corner - 0.5 * sub_len[k];
  }
  for (int k = 0; k < 2; ++k) {  // exit 4: the requested centre in the submap's own geometry
    const Axis sub = {size[k], resolution, sub_len[k], sub_pos[k]};
    if (!inside(sub, req[k])) return TE_OK;
  }
  // (a centre inside a submap that starts at a cell of the map and ends at a bounded corner: 1 <= size, top-left + size <= n;
  // the callers that index memory with the plan check it again, te_submap.hip)
  out->ok = 1;
  out->row0 = tl[0];
  out->col0 = tl[1];
  out->rows = size[0];
  out->cols = size[1];
  out->pos_x = sub_pos[0];
  out->pos_y = sub_pos[1];
  out->length_x = sub_len[0];
  out->length_y = sub_len[1];
  return TE_OK;
}

}  // namespace submap
}  // namespace te
