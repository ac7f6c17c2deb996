// CPU harness over te_polygon_table.h (the offset table of te_run_polygon_footprint and the inside test of every polygon
// kernel), built with the host compiler by tests/test_polygon_table.py.
//   polygon_table_check
//       a few hundred random 3..8-gons, each as given and turned by a random yaw, on three geometries (below)
//   polygon_table_check check <rows> <cols> <res> <pos_x> <pos_y> <yaw> <x0 y0 ...>
//       the same proof for one footprint of tests/polygon_cases.py (rows, cols and the position are read and not used: the
//       proof runs on its own small maps)
//   polygon_table_check route <rows> <cols> <res> <pos_x> <pos_y> <yaw> <x0 y0 ...>
//       which kernel te_run_polygon_footprint launches for this footprint on this map.  Two lines, polygon 0 (as given) and
//       polygon 1 (turned by yaw):  "table|percell fits|extent|span|tile di_span dj_span n_rows n_uncertain tile_bytes"
//       (percell: the limit that refused it; the spans are then the ones that did not fit).  One polygon that does not fit
//       sends BOTH to the per-cell kernel; the third line says which kernel runs: "kernel table|percell".
// The proof, for one footprint (vertex offsets from the centre cell) on one geometry of at most 40 x 40 cells, for EVERY
// centre cell of the map:
//   walk    walking the table as k_polygon_footprint_table does -- rows, items, runs clipped to the map, "uncertain" items
//           evaluated with the exact expression inside the bounding box -- gives exactly the cells, in exactly the order, that
//           polygon_bbox plus polygon_inside give (what k_polygon_footprint, k_polygons_traversable and the oracle walk)
//   inside  no offset of a run ("inside for every centre cell") is outside by the exact expression, or outside the box
//   outside no cell the table does not list is inside by the exact expression
//   tile    every LDS index the walk forms for lane 0 and lane 255 lies inside the staged tile
//   quad    Quad::inside == polygon_inside for n == 4, at every cell the walk tests
// The three geometries: origin (0.7, -0.2); an origin far from zero (500, -500: tests/conditioning_cases.py FAR); and a
// resolution of 0.01 -- the footprint keeps its shape in cells there.  Ends with "N checks, 0 failed checks".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <utility>
#include <vector>

#include "te_polygon_table.h"

using namespace te;

static long g_checks = 0, g_failed = 0;
static void check(bool ok, const char* what, int a = 0, int b = 0, int c = 0) {
  ++g_checks;
  if (ok) return;
  if (++g_failed <= 20) printf("FAILED %s (%d %d %d)\n", what, a, b, c);
}

static Geo make_geo(int rows, int cols, double res, double pos_x, double pos_y) {  // te_set_geometry
  Geo g;
  g.rows = rows;
  g.cols = cols;
  g.batch = 1;
  g.res = res;
  g.len_x = (double)rows * res;
  g.len_y = (double)cols * res;
  g.pos_x = pos_x;
  g.pos_y = pos_y;
  g.ax = pos_x + (0.5 * g.len_x - 0.5 * res);
  g.ay = pos_y + (0.5 * g.len_y - 0.5 * res);
  return g;
}

typedef std::vector<std::pair<int, int>> Cells;

// k_polygon_footprint_table's walk for the centre cell (i, j); `tested`: the cells whose inside test it evaluated
static void walk_table(const Geo& g, int n, const double* off, const PolygonTable& tb, const unsigned* stream, int i, int j, Cells& out,
                       Cells& tested) {
  const double cx = cell_x(g, i), cy = cell_y(g, j);
  auto vert = [&](int k, double& x, double& y) {
    x = off[2 * k] + cx;
    y = off[2 * k + 1] + cy;
  };
  const int W = 255 + tb.di_span;
  const long tile = (long)W * tb.dj_span;
  int ti = 0, bi = -1, tj = 0, bj = -1;
  Quad quad = {};
  if (tb.n_uncertain) {
    polygon_bbox(g, n, vert, ti, bi, tj, bj);
    if (n == 4) quad.load(vert);
  }
  const unsigned* p = stream + tb.first;
  for (int r = 0; r < tb.n_rows; ++r) {
    const unsigned hdr = *p++;
    const int di_idx = hdr & 0xff, items = hdr >> 8;
    const int aa = i + tb.di_min + di_idx;
    const bool a_in = aa >= 0 && aa < g.rows;
    check(di_idx < tb.di_span, "tile: row index beyond di_span", di_idx, tb.di_span);
    for (int k = 0; k < items; ++k) {
      const unsigned item = *p++;
      const int dj_idx = item & 0xff, len = (item >> 8) & 0xff;
      const int b0 = j + tb.dj_min + dj_idx;
      // lanes 0 and 255 of the workgroup: tile + tid + di_idx + (dj_idx + m) * W, m < len
      check(len >= 1 && (long)255 + di_idx + (long)(dj_idx + len - 1) * W < tile, "tile: an item reads beyond the tile", di_idx, dj_idx, len);
      if (!(item >> 31)) {
        for (int m = 0; m < len; ++m)
          if (a_in && b0 + m >= 0 && b0 + m < g.cols) out.push_back({aa, b0 + m});  // (off the map the tile holds +0.0 and ncells skips it)
      } else {
        check(len == 1, "an uncertain item is one cell", len);
        if (a_in && b0 >= 0 && b0 < g.cols && aa >= ti && aa <= bi && b0 >= tj && b0 <= bj) {
          tested.push_back({aa, b0});
          if (n == 4 ? quad.inside(cell_x(g, aa), cell_y(g, b0)) : polygon_inside(n, vert, cell_x(g, aa), cell_y(g, b0))) out.push_back({aa, b0});
        }
      }
    }
  }
}

// class of every offset of the table: 0 not listed, 1 in a run, 2 uncertain
static std::vector<signed char> table_classes(const PolygonTable& tb, const unsigned* stream) {
  std::vector<signed char> cls((size_t)tb.di_span * tb.dj_span, 0);
  const unsigned* p = stream + tb.first;
  for (int r = 0; r < tb.n_rows; ++r) {
    const unsigned hdr = *p++;
    const int di_idx = hdr & 0xff, items = hdr >> 8;
    for (int k = 0; k < items; ++k) {
      const unsigned item = *p++;
      const int dj_idx = item & 0xff, len = (item >> 8) & 0xff;
      for (int m = 0; m < len; ++m)
        if (di_idx < tb.di_span && dj_idx + m < tb.dj_span) cls[(size_t)di_idx * tb.dj_span + dj_idx + m] = (item >> 31) ? 2 : 1;
    }
  }
  return cls;
}

// the proof for one polygon (vertex offsets) on one geometry; returns false when the table format refused it
static bool prove_one(const Geo& g, int n, const double* off) {
  std::vector<unsigned> stream(3, 0xdeadbeefu);  // (the table does not start at word 0: tb.first is honoured)
  PolygonTable tb;
  PolygonTableRefusal why;
  const bool fits = build_polygon_table(g, n, off, stream, tb, &why);
  check(fits == (why == kPolygonTableFits), "the refusal names a limit");
  if (!fits) return false;
  check(tb.first == 3 && tb.di_span >= 1 && tb.dj_span >= 1 && tb.di_span <= kPolygonTableMaxSpan && tb.dj_span <= kPolygonTableMaxSpan &&
            polygon_tile_bytes(tb) <= kPolygonTableMaxTile,
        "a table that fits respects the limits", tb.di_span, tb.dj_span);
  const std::vector<signed char> cls = table_classes(tb, stream.data());
  Cells got, want, tested;
  for (int i = 0; i < g.rows; ++i)
    for (int j = 0; j < g.cols; ++j) {
      const double cx = cell_x(g, i), cy = cell_y(g, j);
      auto vert = [&](int k, double& x, double& y) {
        x = off[2 * k] + cx;
        y = off[2 * k + 1] + cy;
      };
      got.clear();
      tested.clear();
      walk_table(g, n, off, tb, stream.data(), i, j, got, tested);
      int ti, bi, tj, bj;
      polygon_bbox(g, n, vert, ti, bi, tj, bj);
      want.clear();
      for (int a = ti; a <= bi; ++a)
        for (int b = tj; b <= bj; ++b)
          if (polygon_inside(n, vert, cell_x(g, a), cell_y(g, b))) want.push_back({a, b});
      check(got == want, "walk: the table's cells and their order", i, j, (int)want.size());
      // inside / outside, offset by offset over the whole map
      for (int a = 0; a < g.rows; ++a)
        for (int b = 0; b < g.cols; ++b) {
          const int da = a - i - tb.di_min, db = b - j - tb.dj_min;
          const int c = (da >= 0 && da < tb.di_span && db >= 0 && db < tb.dj_span) ? cls[(size_t)da * tb.dj_span + db] : 0;
          const bool boxed = a >= ti && a <= bi && b >= tj && b <= bj;
          if (c == 2 || (c == 0 && !boxed)) continue;  // decided per cell; not listed and not walked by the reference either
          const bool exact = boxed && polygon_inside(n, vert, cell_x(g, a), cell_y(g, b));
          if (c == 1)
            check(exact, "inside: a cell of a run is outside by the exact expression", a - i, b - j);
          else
            check(!exact, "outside: a cell the table does not list is inside by the exact expression", a - i, b - j);
        }
      if (n == 4) {
        Quad quad;
        quad.load(vert);
        bool same = true;
        for (const auto& q : tested) same = same && quad.inside(cell_x(g, q.first), cell_y(g, q.second)) == polygon_inside(n, vert, cell_x(g, q.first), cell_y(g, q.second));
        for (int a = ti; a <= bi; ++a)
          for (int b = tj; b <= bj; ++b) same = same && quad.inside(cell_x(g, a), cell_y(g, b)) == polygon_inside(n, vert, cell_x(g, a), cell_y(g, b));
        check(same, "quad: Quad::inside against polygon_inside", i, j);
      }
    }
  return true;
}

// one footprint, as given and turned by yaw, on the three geometries; pts in metres at resolution `res`
static int prove_footprint(int rows, int cols, double res, int n, const double* pts, double yaw) {
  int tables = 0;
  const double geos[3][3] = {{res, 0.7, -0.2}, {res, 500.0, -500.0}, {0.01, 0.7, -0.2}};
  for (const auto& ge : geos) {
    const Geo g = make_geo(rows, cols, ge[0], ge[1], ge[2]);
    std::vector<double> scaled(pts, pts + 2 * n), off(2 * (size_t)n);
    for (double& v : scaled) v = v / res * ge[0];  // the same shape in cells
    for (int which = 0; which < 2; ++which) {
      rotate_footprint(n, scaled.data(), which ? yaw : 0.0, off.data());
      tables += prove_one(g, n, off.data());
    }
  }
  return tables;
}

static int parse_polygon(int argc, char** argv, int& rows, int& cols, double& res, double& px, double& py, double& yaw, std::vector<double>& pts) {
  if (argc < 8 + 2 || ((argc - 8) & 1)) return 2;
  rows = atoi(argv[2]);
  cols = atoi(argv[3]);
  res = atof(argv[4]);
  px = atof(argv[5]);
  py = atof(argv[6]);
  yaw = atof(argv[7]);
  for (int k = 8; k < argc; ++k) pts.push_back(atof(argv[k]));
  if (rows < 1 || cols < 1 || !(res > 0.0) || pts.size() / 2 > 32) return 2;
  return 0;
}

static int route_mode(int argc, char** argv) {
  int rows, cols;
  double res, px, py, yaw;
  std::vector<double> pts;
  if (parse_polygon(argc, argv, rows, cols, res, px, py, yaw, pts)) return 2;
  const int n = (int)(pts.size() / 2);
  const Geo g = make_geo(rows, cols, res, px, py);
  static const char* const kWhy[] = {"fits", "extent", "span", "tile"};
  std::vector<unsigned> stream;
  std::vector<double> off(2 * (size_t)n);
  bool all = true;
  for (int which = 0; which < 2; ++which) {  // (te_run_polygon_footprint stops at the first polygon that does not fit; both are reported here)
    rotate_footprint(n, pts.data(), which ? yaw : 0.0, off.data());
    PolygonTable tb;
    PolygonTableRefusal why;
    const bool fits = build_polygon_table(g, n, off.data(), stream, tb, &why);
    all = all && fits;
    printf("%s %s %d %d %d %d %zu\n", fits ? "table" : "percell", kWhy[why], tb.di_span, tb.dj_span, tb.n_rows, tb.n_uncertain, polygon_tile_bytes(tb));
  }
  printf("kernel %s\n", all ? "table" : "percell");
  return 0;
}

static int check_mode(int argc, char** argv) {
  int rows, cols;
  double res, px, py, yaw;
  std::vector<double> pts;
  if (parse_polygon(argc, argv, rows, cols, res, px, py, yaw, pts)) return 2;
  // (a map with unequal sides: a transposed index shows)
  const int tables = prove_footprint(40, 31, res, (int)(pts.size() / 2), pts.data(), yaw);
  printf("%d tables\n", tables);
  printf("%ld checks, %ld failed checks\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}

static int random_mode() {
  std::mt19937_64 rng(5);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  const double kPi = 3.14159265358979323846;
  int tables = 0, polygons = 0;
  for (int trial = 0; trial < 300; ++trial) {
    const int n = 3 + (int)(rng() % 6);
    const double res = trial % 3 == 0 ? 0.05 : (trial % 3 == 1 ? 0.1 : 0.0373);
    // every fifth tiny (covers no or one cell centre), every seventh with edges through cell centres, the rest up to 9 cells
    double ang[8], pts[16];
    for (int k = 0; k < n; ++k) ang[k] = u(rng) * 2.0 * kPi;
    std::sort(ang, ang + n);
    const double scale = res * (trial % 5 == 0 ? 0.4 : 1.5 + 7.5 * u(rng));
    for (int k = 0; k < n; ++k) {
      const double rad = scale * (0.4 + 0.6 * u(rng));
      pts[2 * k] = rad * cos(ang[k]);
      pts[2 * k + 1] = rad * sin(ang[k]);
      if (trial % 7 == 0) {
        pts[2 * k] = res * 0.5 * floor(pts[2 * k] / res * 2.0 + 0.5);
        pts[2 * k + 1] = res * 0.5 * floor(pts[2 * k + 1] / res * 2.0 + 0.5);
      }
    }
    const double yaw = trial % 4 == 0 ? kPi / 2 : (u(rng) - 0.5) * 2.0 * kPi;
    tables += prove_footprint(23 + trial % 11, 17 + trial % 13, res, n, pts, yaw);
    polygons += 6;
  }
  check(tables > polygons / 2, "most random polygons fit the table", tables, polygons);
  printf("%d polygons, %d tables\n", polygons, tables);
  printf("%ld checks, %ld failed checks\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "route")) return route_mode(argc, argv);
  if (argc >= 2 && !strcmp(argv[1], "check")) return check_mode(argc, argv);
  if (argc == 1) return random_mode();
  fprintf(stderr, "usage: polygon_table_check [route|check <rows> <cols> <res> <pos_x> <pos_y> <yaw> <x0 y0 ...>]\n");
  return 2;
}
