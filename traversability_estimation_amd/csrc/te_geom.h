// te_geom.h -- grid_map_core geometry on the device: cell centres, checkIfPositionWithinMap,
// getIndexFromPosition (both in te_polygon_table.h) and the Bresenham LineIterator, in the reference's own double arithmetic.
// (te_path_visit.h holds a plain C++ copy of pos_inside, pos_to_index and LineIt -- pv::Geom, for the host driver's sizing and
// the CPU check of the visit plan: a change here or there is a change in both.  te_check_footprint_paths_radius compares the
// two walks' visit counts on every call.)
#pragma once
#include "te_internal.h"

namespace te {

// cell_x, cell_y, pos_inside (checkIfPositionWithinMap) and pos_to_index (getIndexFromPosition): te_polygon_table.h, which
// te_internal.h includes -- plain C++ for the host and the device, so that the CPU check of the polygon table runs them too.

// grid_map::LineIterator (Bresenham from (si,sj) to (ei,ej), both included)
struct LineIt {
  int i, j, inc1i, inc1j, inc2i, inc2j, den, num, numadd, ncells, icell;
  __device__ __forceinline__ void init(int si, int sj, int ei, int ej) {
    icell = 0;
    i = si;
    j = sj;
    const int dx = ei > si ? ei - si : si - ei, dy = ej > sj ? ej - sj : sj - ej;
    inc1i = inc2i = (ei >= si) ? 1 : -1;
    inc1j = inc2j = (ej >= sj) ? 1 : -1;
    if (dx >= dy) {
      inc1i = 0;
      inc2j = 0;
      den = dx;
      num = dx / 2;
      numadd = dy;
      ncells = dx + 1;
    } else {
      inc2i = 0;
      inc1j = 0;
      den = dy;
      num = dy / 2;
      numadd = dx;
      ncells = dy + 1;
    }
  }
  __device__ __forceinline__ bool past_end() const { return icell >= ncells; }
  __device__ __forceinline__ void next() {
    num += numadd;
    if (num >= den) {
      num -= den;
      i += inc1i;
      j += inc1j;
    }
    i += inc2i;
    j += inc2j;
    icell++;
  }
};

}  // namespace te
