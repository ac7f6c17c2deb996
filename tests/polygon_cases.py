"""The footprints of the polygon tests, with the kernel each of them takes.

te_run_polygon_footprint has two kernels with identical results: the offset table with its LDS tile, and the kernel that
evaluates every cell of every bounding box.  build_polygon_table (csrc/te_polygon_table.h) decides: a footprint whose box of
offsets spans more than 255 along an axis, or whose tile (255 + di_span) * dj_span * 8 bytes exceeds 64 KiB, does not fit the
table, and ONE polygon of the two (as given, turned by yaw) that does not fit sends both to the per-cell kernel.

A plain module (no fixtures, no conftest).  Each case CLAIMS its route: `kernel`, and per polygon (fits | the limit that refused
it, di_span, dj_span, tile bytes).  tests/test_polygon_table.py asserts every claim through the builder's own code on the
CPU (tests/cpu/polygon_table_check.cpp, mode `route`), so a GPU test of tests/test_gpu_polygon_cases.py or
tests/test_polygon.py can never silently run the other kernel; the same program proves the table of every case against the
bounding box plus the inside test (mode `check`).

Sizes.  With s = di_span = dj_span a square tile fits up to (255 + 28) * 28 * 8 = 63 392 bytes, one row of 2 264 bytes below
the limit; 29 cells a side need 65 888.  A one-cell-wide sliver along y fits up to 256 * 32 * 8 = 65 536 bytes exactly.  The box
of offsets has a margin of one cell and one rounding step on either side, so a sliver of c cells has a box of c + 4: 251 cells
are the longest that fit (row indices up to 250, W = 255 + 251 = 506), 252 the first that do not.
"""
import math

import numpy as np

POS = (0.7, -0.2)  # the map position of every route claim, and of the GPU tests that run the cases
FOOTPRINT = [[0.45, 0.30], [0.45, -0.30], [-0.45, -0.30], [-0.45, 0.30]]  # robot_footprint_parameter.yaml:3
POINTS_XYZ = [[0.45, 0.30, 0.0], [0.45, -0.30, 0.0], [-0.45, -0.30, 0.0], [-0.45, 0.30, 0.0]]


def terrain(rows, cols, seed, holes=0.02, boxes=6, amplitude=0.5):
    from traversability_estimation_amd import synth
    e = synth.perlin_elevation(rows, cols, seed=seed, amplitude=amplitude)
    if boxes and rows > 8 and cols > 8:
        e = synth.with_steps(e, boxes, seed=seed + 1)
    if holes:
        e = synth.with_holes(e, holes, seed=seed + 2)
    return np.ascontiguousarray(e, dtype=np.float32).reshape(-1)


def rect(res, x_lo, x_hi, y_lo, y_hi):
    """A rectangle given in cells: it covers the offsets di with x_lo < -di < x_hi, likewise dj."""
    return [[x_hi * res, y_hi * res], [x_hi * res, y_lo * res], [x_lo * res, y_lo * res], [x_lo * res, y_hi * res]]


def fits(di_span, dj_span):
    return ("fits", di_span, dj_span, (255 + di_span) * dj_span * 8)


# ---- the eight cases of tests/test_polygon.py::test_polygon_footprint_layers, in its order ------------------------------------
EXISTING = [
    dict(rows=100, cols=133, res=0.03, pts=FOOTPRINT, yaw=math.pi / 2, kernel="percell",
         polygons=[fits(31, 21), ("tile", 21, 31, 68448)]),  # turned by pi / 2 its 31 columns need 68 448 bytes: BOTH polygons go per cell
    dict(rows=150, cols=70, res=0.05, pts=FOOTPRINT, yaw=0.4, kernel="table", polygons=[fits(19, 13), fits(21, 17)]),
    dict(rows=64, cols=64, res=0.05, pts=[[0.3, 0.0], [-0.2, 0.25], [-0.2, -0.25]], yaw=-2.2, kernel="table",
         polygons=[fits(11, 11), fits(9, 10)]),
    dict(rows=61, cols=90, res=0.04, pts=[[0.3, 0.3], [0.3, -0.3], [0.0, -0.3], [0.0, 0.0], [-0.3, 0.0], [-0.3, 0.3]], yaw=1.0,
         kernel="table", polygons=[fits(15, 15), fits(21, 17)]),
    dict(rows=33, cols=20, res=0.1, pts=[[0.01, 0.01], [0.01, -0.01], [-0.01, -0.01]], yaw=0.3, kernel="table",
         polygons=[fits(1, 1), fits(1, 1)]),  # covers no cell centre
    dict(rows=5, cols=7, res=0.1, pts=FOOTPRINT, yaw=0.9, kernel="table", polygons=[fits(9, 7), fits(9, 9)]),  # footprint larger than the map
    dict(rows=300, cols=40, res=0.05, pts=FOOTPRINT, yaw=math.pi / 2, kernel="table", polygons=[fits(19, 13), fits(13, 19)]),  # several workgroups along the rows
    dict(rows=120, cols=60, res=0.02, pts=[[0.72, 0.48], [0.72, -0.48], [-0.72, -0.48], [-0.72, 0.48]], yaw=0.3,
         over=dict(fp_radius=0.2, fp_offset=0.1), kernel="percell",
         polygons=[("tile", 73, 49, 128576), ("tile", 83, 67, 181168)]),  # 72 x 48 cells: too large for the offset table
]
for _k, _c in enumerate(EXISTING):
    _c["name"] = "existing%d" % _k

# ---- the table's format limits ----------------------------------------------------------------------------------------------------
RES = 0.05
LIMITS = [
    # the largest square tile that fits: 28 x 28 cells, 2 144 bytes below the limit (one row of the tile is 2 264)
    dict(name="lds_fits", rows=300, cols=40, res=RES, pts=rect(RES, -13.75, 14.25, -13.75, 14.25), yaw=math.pi / 2, kernel="table",
         polygons=[fits(28, 28), fits(28, 28)]),
    # one cell larger
    dict(name="lds_over", rows=300, cols=40, res=RES, pts=rect(RES, -14.25, 14.75, -14.25, 14.75), yaw=math.pi / 2, kernel="percell",
         polygons=[("tile", 29, 29, 65888), ("tile", 29, 29, 65888)]),
    # the longest sliver along x that fits: 251 cells, row indices up to 250, W = 506
    dict(name="long_x", rows=520, cols=12, res=RES, pts=rect(RES, -125.25, 125.75, -0.4, 0.4), yaw=math.pi, kernel="table",
         polygons=[fits(251, 1), fits(251, 1)]),
    # the first that does not, and the issue's 254 cells
    dict(name="long_x_252", rows=520, cols=12, res=RES, pts=rect(RES, -125.75, 126.25, -0.4, 0.4), yaw=math.pi, kernel="percell",
         polygons=[("span", 256, 5, 0), ("span", 256, 5, 0)]),
    dict(name="long_x_over", rows=520, cols=12, res=RES, pts=rect(RES, -126.75, 127.25, -0.4, 0.4), yaw=math.pi, kernel="percell",
         polygons=[("span", 258, 5, 0), ("span", 258, 5, 0)]),
    # a one-cell-wide sliver along y at the largest dj_span there is: 32 columns, a tile of exactly 65 536 bytes
    dict(name="long_y", rows=300, cols=48, res=RES, pts=rect(RES, -0.4, 0.4, -15.75, 16.25), yaw=math.pi, kernel="table",
         polygons=[fits(1, 32), fits(1, 32)]),
    dict(name="long_y_over", rows=300, cols=48, res=RES, pts=rect(RES, -0.4, 0.4, -16.25, 16.75), yaw=math.pi, kernel="percell",
         polygons=[("tile", 1, 33, 67584), ("tile", 1, 33, 67584)]),
    # three cells wide: dj_span 31 is the most for di_span 2 and 3
    dict(name="long_y_3", rows=300, cols=48, res=RES, pts=rect(RES, -1.4, 1.4, -15.25, 15.75), yaw=math.pi, kernel="table",
         polygons=[fits(3, 31), fits(3, 31)]),
    # the yaw decides: 40 cells along x fit (di_span 40, one column), turned by pi / 2 they are 40 columns of 256 rows
    dict(name="yaw_mixed", rows=300, cols=48, res=RES, pts=rect(RES, -19.75, 20.25, -0.4, 0.4), yaw=math.pi / 2, kernel="percell",
         polygons=[fits(40, 1), ("tile", 1, 40, 81920)]),
]

CASES = EXISTING + LIMITS


def case(name):
    return next(c for c in CASES if c["name"] == name)


def route_args(c):
    """The arguments of `polygon_table_check route|check` for a case."""
    return [c["rows"], c["cols"], repr(float(c["res"])), repr(POS[0]), repr(POS[1]), repr(float(c["yaw"]))] + \
        [repr(float(v)) for pt in c["pts"] for v in pt]


# the terrain each limit case runs on: gentle, with few kerbs -- a footprint of 28 x 28 cells finds an untraversable cell
# almost everywhere on the terrain of the other tests.  Chosen on the CPU so that the oracle alone gives both outcomes.
def limit_terrain(c):
    return terrain(c["rows"], c["cols"], seed=c.get("seed", 3), holes=0.002, boxes=c.get("boxes", 3), amplitude=0.1)
