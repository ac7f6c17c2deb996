// te_path_walk.h -- checkCircularFootprintPath (TraversabilityMap.cpp:344-462) for one path on the device, shared by the two
// circular path kernels: k_check_circular_paths (te_paths.hip: a centre's value is read from the complete footprint layer, the
// memo branch :672-677 of isTraversable) and k_pd_paths (te_path_discs.hip: looked up among the discs evaluated on demand).
// Status codes, checkInclination, the nSkip = 3 walk and the length-weighted mean live here once.
#pragma once
#include "te_geom.h"
#include "te_internal.h"

namespace te {

// TraversabilityMap::checkInclination(start, end) :748-762.  outside: a position off the map -- atPosition throws
// there, and the segment branch ignores getIndex()'s failure (undefined indices); reported as status 1.
__device__ __forceinline__ bool inclination_ok(const Geo& g, const float* __restrict__ robot_slope, double sx, double sy,
                                               double ex, double ey, bool& outside) {
  int si, sj, ei, ej;
  outside = false;
  if (ex == sx && ey == sy) {  // :750-751
    if (!pos_inside(g, sx, sy) || !pos_to_index(g, sx, sy, si, sj)) {
      outside = true;
      return false;
    }
    return !((double)robot_slope[(size_t)sj * g.rows + si] == 0.0);
  }
  if (!pos_to_index(g, sx, sy, si, sj) || !pos_to_index(g, ex, ey, ei, ej)) {
    outside = true;
    return false;
  }
  LineIt L;
  for (L.init(si, sj, ei, ej); !L.past_end(); L.next()) {  // from the start index to the end index :756
    const float v = robot_slope[(size_t)L.j * g.rows + L.i];
    if (!isfinite(v)) continue;  // isValid :757
    if ((double)v == 0.0) return false;
  }
  return true;
}

// One path of n poses xy[2n]; value_at(i, j): isTraversable's value at the centre cell (i, j) as a double (traversable: != 0).
// robot_slope: the layer checkInclination reads (nullptr: footprint/check_robot_inclination off).
template <class V>
__device__ __forceinline__ void check_circular_path(const Geo& g, const float* __restrict__ robot_slope, double fp_default, int n,
                                                    const double* __restrict__ xy, V&& value_at, unsigned char& safe_out, double& trav_out,
                                                    int& status_out) {
  unsigned char safe = 0;
  double out = 0.0;
  int st = 0;
  if (n <= 0) {  // :330-334
    st = 2;
  } else {
    double res_trav = 0.0, length_path = 0.0, ex = 0.0, ey = 0.0;
    bool ok = true;
    for (int i = 0; i < n && ok; ++i) {
      const double sx = ex, sy = ey;
      ex = xy[2 * i];
      ey = xy[2 * i + 1];
      if (robot_slope && (n == 1 || i > 0)) {  // checkRobotInclination_ :366-370, :390-394
        bool outside;
        const bool good = n == 1 ? inclination_ok(g, robot_slope, ex, ey, ex, ey, outside)
                                 : inclination_ok(g, robot_slope, sx, sy, ex, ey, outside);
        if (!good) {
          st = outside ? 1 : 0;
          ok = false;
          break;
        }
      }
      if (n == 1) {  // :365-385
        double t = fp_default;
        if (pos_inside(g, ex, ey)) {  // :663-665 otherwise
          int ci, cj;
          pos_to_index(g, ex, ey, ci, cj);
          t = value_at(ci, cj);
        }
        if (!(t != 0.0)) {
          ok = false;
          break;
        }
        res_trav = t;
      }
      if (n > 1 && i > 0) {  // :388-456
        int si, sj, ei, ej;
        if (!pos_to_index(g, sx, sy, si, sj) || !pos_to_index(g, ex, ey, ei, ej)) {
          st = 1;  // the reference ignores getIndex()'s result here: undefined indices
          ok = false;
          break;
        }
        double sum = 0.0;
        int nline = 0;
        LineIt L;
        for (L.init(ei, ej, si, sj); !L.past_end(); L.next()) {  // from the end index to the start index
          const double t = value_at(L.i, L.j);
          if (!(t != 0.0)) {
            ok = false;
            break;
          }
          sum += t;
          nline++;
          for (int s = 0; s < 3; ++s)  // nSkip :396
            if (!L.past_end()) L.next();
        }
        if (!ok) break;
        const double t = sum / (double)nline;
        const double dx = ex - sx, dy = ey - sy;
        const double length_segment = sqrt(dx * dx + dy * dy);
        if (i > 1) {  // :443-447
          const double length_previous = length_path;
          length_path += length_segment;
          res_trav = (length_segment * t + length_previous * res_trav) / length_path;
        } else {
          length_path = length_segment;
          res_trav = t;
        }
      }
    }
    if (ok) {
      safe = 1;
      out = res_trav;
    }
  }
  safe_out = safe;
  trav_out = out;
  status_out = st;
}

}  // namespace te
