// te_polygon_table.h -- what the polygon footprint kernels (te_polygon.hip) decide before they read a layer: the cells a
// polygon covers (grid_map::PolygonIterator: bounding box, then Polygon::isInside's crossing number), and the offset table
// of te_run_polygon_footprint with the limits of its format (build_polygon_table: spans of at most 255 offsets, an LDS
// tile of at most 64 KiB; a footprint beyond either takes the per-cell kernel).
//
// Plain C++ that compiles for the host and the device, in a header of its own: the kernels instantiate exactly this text,
// and the CPU check (tests/cpu/polygon_table_check.cpp, tests/test_polygon_table.py) walks the table as
// k_polygon_footprint_table does, against the bounding box plus the inside test, and reports which route a footprint
// takes -- the claim tests/polygon_cases.py makes for every case the GPU tests run.
//
// It also holds the map geometry (Geo) and grid_map_core's cell arithmetic (cell centres, checkIfPositionWithinMap,
// getIndexFromPosition) in the reference's own double arithmetic; te_geom.h adds the line iterator for the kernels.
// (te_path_visit.h holds a plain C++ copy of pos_inside and pos_to_index -- pv::Geom: a change here is a change there.)
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define TE_PT_HD __host__ __device__ __forceinline__
#else
#define TE_PT_HD inline
#endif

namespace te {

// Map geometry as the kernels need it.  Device layout of every layer: [batch][cols][rows] float32,
// i.e. grid_map's column-major matrix; the FAST axis is the grid_map row index i ("x" below).
struct Geo {
  int rows, cols, batch;
  double res;
  double ax, ay;  // position of cell 0: pos + (0.5*len - 0.5*res); x(i) = ax + res*(-i)
  double len_x, len_y, pos_x, pos_y;
};

TE_PT_HD double cell_x(const Geo& g, int i) { return g.ax + g.res * (double)(-i); }
TE_PT_HD double cell_y(const Geo& g, int j) { return g.ay + g.res * (double)(-j); }

// checkIfPositionWithinMap (grid_map_core)
TE_PT_HD bool pos_inside(const Geo& g, double x, double y) {
  const double tx = -((x - g.pos_x) - 0.5 * g.len_x);
  const double ty = -((y - g.pos_y) - 0.5 * g.len_y);
  return tx >= 0.0 && ty >= 0.0 && tx < g.len_x && ty < g.len_y;
}
// getIndexFromPosition (grid_map_core)
TE_PT_HD bool pos_to_index(const Geo& g, double x, double y, int& i, int& j) {
  const double vx = ((x - 0.5 * g.len_x) - g.pos_x) / g.res;
  const double vy = ((y - 0.5 * g.len_y) - g.pos_y) / g.res;
  i = (int)(-vx);
  j = (int)(-vy);
  return pos_inside(g, x, y) && i >= 0 && j >= 0 && i < g.rows && j < g.cols;
}

// offset table of one footprint polygon (build_polygon_table): rows of the bounding box that hold cells, each a header
// word (di index | items << 8) followed by its items (dj index | run length << 8 | "decided per cell" << 31)
struct PolygonTable {
  int first;              // index of the first word in the stream
  int n_rows;
  int n_uncertain;
  int di_min, dj_min;     // offset of table index 0
  int di_span, dj_span;   // extent of the staged tile in offsets
};
struct PolygonTables {
  PolygonTable t[2];
};

// the limits of the table format
constexpr int kPolygonTableMaxSpan = 255;               // offsets along either axis (8-bit indices, 8-bit run lengths)
constexpr size_t kPolygonTableMaxTile = 64 * 1024;      // bytes of the staged tile (dynamic LDS of one workgroup)
// why build_polygon_table refused a footprint
enum PolygonTableRefusal { kPolygonTableFits = 0, kPolygonTableExtent = 1, kPolygonTableSpan = 2, kPolygonTableTile = 3 };

// bytes of the tile k_polygon_footprint_table stages: 256 centre cells and the offsets around them, dj_span columns of doubles
TE_PT_HD size_t polygon_tile_bytes(const PolygonTable& tb) { return (size_t)(255 + tb.di_span) * tb.dj_span * sizeof(double); }

// boundPositionToRange (grid_map_core GridMapMath.cpp) for one axis
TE_PT_HD double bound_axis(double position, double len, double mappos) {
  double shifted = position - mappos + 0.5 * len;
  double eps = 10.0 * 2.220446049250313e-16;
  if (fabs(position) > 1.0) eps *= fabs(position);
  if (shifted <= 0)
    shifted = eps;
  else if (shifted >= len)
    shifted = len - eps;
  return shifted + mappos - 0.5 * len;
}

TE_PT_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one edge (xi, yi) - (xj, yj) of grid_map::Polygon::isInside's crossing-number test
TE_PT_HD bool edge_crosses(double xi, double yi, double xj, double yj, double px, double py) {
  if ((yi > py) == (yj > py)) return false;
  if (xi == xj) return px < xi;  // the expression below is 0 * (..) / (..) + xi == xi exactly (yj != yi here)
  const double lo = fmin(xi, xj), hi = fmax(xi, xj);
  const double margin = 1e-9 * (fabs(lo) + fabs(hi) + 1.0);  // >> the rounding error of the expression below
  if (px < lo - margin) return true;
  return px <= hi + margin && px < (xj - xi) * (py - yi) / (yj - yi) + xi;
}

// vert(k, x, y): vertex k of the polygon
template <class V>
TE_PT_HD bool polygon_inside(int n, V&& vert, double px, double py) {
  int cross = 0;
  double xj, yj;
  vert(n - 1, xj, yj);
  for (int i = 0; i < n; ++i) {
    double xi, yi;
    vert(i, xi, yi);
    cross += edge_crosses(xi, yi, xj, yj, px, py);
    xj = xi;
    yj = yi;
  }
  return (cross & 1) != 0;
}

// The usual footprint has four vertices: held in registers, a cell evaluation does not wait for per-edge loads.
struct Quad {
  double x[4], y[4];
  template <class V>
  TE_PT_HD void load(V&& vert) {
    vert(0, x[0], y[0]);
    vert(1, x[1], y[1]);
    vert(2, x[2], y[2]);
    vert(3, x[3], y[3]);
  }
  TE_PT_HD bool inside(double px, double py) const {  // edges (0,3) (1,0) (2,1) (3,2) like the loop
    const int cross = (int)edge_crosses(x[0], y[0], x[3], y[3], px, py) + (int)edge_crosses(x[1], y[1], x[0], y[0], px, py) +
                      (int)edge_crosses(x[2], y[2], x[1], y[1], px, py) + (int)edge_crosses(x[3], y[3], x[2], y[2], px, py);
    return (cross & 1) != 0;
  }
};

// PolygonIterator::findSubmapParameters: the index range [ti, bi] x [tj, bj] the iterator walks
template <class V>
TE_PT_HD void polygon_bbox(const Geo& g, int n, V&& vert, int& ti, int& bi, int& tj, int& bj) {
  double tlx, tly;
  vert(0, tlx, tly);
  double brx = tlx, bry = tly;
  for (int k = 1; k < n; ++k) {
    double x, y;
    vert(k, x, y);
    tlx = tlx < x ? x : tlx;
    tly = tly < y ? y : tly;
    brx = x < brx ? x : brx;
    bry = y < bry ? y : bry;
  }
  tlx = bound_axis(tlx, g.len_x, g.pos_x);
  tly = bound_axis(tly, g.len_y, g.pos_y);
  brx = bound_axis(brx, g.len_x, g.pos_x);
  bry = bound_axis(bry, g.len_y, g.pos_y);
  pos_to_index(g, tlx, tly, ti, tj);
  pos_to_index(g, brx, bry, bi, bj);
  ti = clampi(ti, 0, g.rows - 1);
  bi = clampi(bi, 0, g.rows - 1);
  tj = clampi(tj, 0, g.cols - 1);
  bj = clampi(bj, 0, g.cols - 1);
}

// The rotation part of  toPosition * orientation * positionToVertex  (TraversabilityMap.cpp:250-283) for a yaw-only
// orientation: kindr AngleAxis(yaw, 0, 0, 1) -> quaternion (cos(yaw/2), 0, 0, sin(yaw/2)), Eigen's toRotationMatrix,
// linear * v.  Host side, once per call.
inline void rotate_footprint(int n_points, const double* points_xy, double yaw, double* out_xy) {
  const double w = cos(yaw / 2.0), z = sin(yaw / 2.0);
  const double tz = 2.0 * z, twz = tz * w, tzz = tz * z;
  const double r00 = 1.0 - (0.0 + tzz), r01 = 0.0 - twz, r10 = 0.0 + twz, r11 = 1.0 - (0.0 + tzz);
  for (int k = 0; k < n_points; ++k) {
    const double px = points_xy[2 * k], py = points_xy[2 * k + 1];
    out_xy[2 * k] = r00 * px + r01 * py;
    out_xy[2 * k + 1] = r10 * px + r11 * py;
  }
}

// Classify the index offsets (di, dj) of one footprint polygon (vertex offsets `off` from the centre cell).  The cell at
// offset (di, dj) lies at (-di, -dj) * res from the centre.  Returns false when the polygon does not fit the table
// format (spans beyond 255 offsets, LDS tile too large): the caller then uses the per-cell kernel.  `why` (optional): which
// limit refused it; the spans of `tb` are then the ones that did not fit.
inline bool build_polygon_table(const Geo& g, int n, const double* off, std::vector<unsigned>& stream, PolygonTable& tb,
                                PolygonTableRefusal* why = nullptr) {
  auto refuse = [&](PolygonTableRefusal r) {
    if (why) *why = r;
    return false;
  };
  if (why) *why = kPolygonTableFits;
  double xmin = off[0], xmax = off[0], ymin = off[1], ymax = off[1], ext = 0.0;
  for (int k = 0; k < n; ++k) {
    xmin = std::min(xmin, off[2 * k]);
    xmax = std::max(xmax, off[2 * k]);
    ymin = std::min(ymin, off[2 * k + 1]);
    ymax = std::max(ymax, off[2 * k + 1]);
    ext = std::max(ext, std::max(fabs(off[2 * k]), fabs(off[2 * k + 1])));
  }
  // rounding of the per-cell evaluation is ~1e-16 of the coordinates involved; anything closer than `tol` to an edge
  // is left to that evaluation
  const double scale = fabs(g.pos_x) + fabs(g.pos_y) + g.len_x + g.len_y + ext;
  const double tol = 1e-7 * g.res + 1e-9 * scale;
  tb.first = (int)stream.size();
  tb.n_rows = tb.n_uncertain = tb.di_min = tb.dj_min = tb.di_span = tb.dj_span = 0;
  if (!(ext / g.res < 1e6)) return refuse(kPolygonTableExtent);  // far beyond any table; also keeps the casts below defined
  const int di_lo = (int)floor(-xmax / g.res) - 1, di_hi = (int)ceil(-xmin / g.res) + 1;
  const int dj_lo = (int)floor(-ymax / g.res) - 1, dj_hi = (int)ceil(-ymin / g.res) + 1;
  if (di_hi - di_lo + 1 > kPolygonTableMaxSpan || dj_hi - dj_lo + 1 > kPolygonTableMaxSpan) {
    tb.di_span = di_hi - di_lo + 1;
    tb.dj_span = dj_hi - dj_lo + 1;
    return refuse(kPolygonTableSpan);
  }
  auto classify = [&](int di, int dj) {  // 0 outside, 1 inside, 2 decided by rounding
    const double px = -(double)di * g.res, py = -(double)dj * g.res;
    int cross = 0;
    double dmin = 1e300;
    for (int i = 0, j = n - 1; i < n; j = i++) {
      const double xi = off[2 * i], yi = off[2 * i + 1], xj = off[2 * j], yj = off[2 * j + 1];
      if (((yi > py) != (yj > py)) && (px < (xj - xi) * (py - yi) / (yj - yi) + xi)) cross++;
      const double ex = xj - xi, ey = yj - yi, l2 = ex * ex + ey * ey;
      double u = l2 > 0.0 ? ((px - xi) * ex + (py - yi) * ey) / l2 : 0.0;
      u = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
      const double qx = xi + u * ex - px, qy = yi + u * ey - py;
      dmin = std::min(dmin, sqrt(qx * qx + qy * qy));
    }
    if (!(dmin > tol)) return 2;
    return cross & 1;
  };
  // the used part of the box
  int a0 = di_hi + 1, a1 = di_lo - 1, b0 = dj_hi + 1, b1 = dj_lo - 1;
  std::vector<signed char> cls((size_t)(di_hi - di_lo + 1) * (dj_hi - dj_lo + 1));
  for (int di = di_lo; di <= di_hi; ++di)
    for (int dj = dj_lo; dj <= dj_hi; ++dj) {
      const int c = classify(di, dj);
      cls[(size_t)(di - di_lo) * (dj_hi - dj_lo + 1) + (dj - dj_lo)] = (signed char)c;
      if (c) {
        a0 = std::min(a0, di);
        a1 = std::max(a1, di);
        b0 = std::min(b0, dj);
        b1 = std::max(b1, dj);
      }
    }
  if (a1 < a0) {  // covers no cell centre
    tb.di_min = tb.dj_min = 0;
    tb.di_span = tb.dj_span = 1;
    return true;
  }
  tb.di_min = a0;
  tb.dj_min = b0;
  tb.di_span = a1 - a0 + 1;
  tb.dj_span = b1 - b0 + 1;
  if (polygon_tile_bytes(tb) > kPolygonTableMaxTile) return refuse(kPolygonTableTile);
  for (int di = a0; di <= a1; ++di) {  // SubmapIterator order: row index outer, column index inner
    const size_t hdr = stream.size();
    stream.push_back(0);
    unsigned items = 0;
    for (int dj = b0; dj <= b1;) {
      const int c = cls[(size_t)(di - di_lo) * (dj_hi - dj_lo + 1) + (dj - dj_lo)];
      if (c == 0) {
        ++dj;
        continue;
      }
      int len = 1;
      if (c == 1)
        while (dj + len <= b1 && len < 255 && cls[(size_t)(di - di_lo) * (dj_hi - dj_lo + 1) + (dj + len - dj_lo)] == 1) ++len;
      else
        ++tb.n_uncertain;
      stream.push_back((unsigned)(dj - b0) | ((unsigned)len << 8) | (c == 2 ? 0x80000000u : 0u));
      ++items;
      dj += len;
    }
    if (items == 0) {
      stream.pop_back();
      continue;
    }
    stream[hdr] = (unsigned)(di - a0) | (items << 8);
    ++tb.n_rows;
  }
  return true;
}

}  // namespace te
