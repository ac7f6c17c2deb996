"""The shapes, caps and inputs of tests/test_gpu_distance.py, kept apart from it so that tests/test_distance_plan.py can check --
without a GPU -- that every case takes the route its GPU test claims."""
import numpy as np

from tests import median_fill_cases as M

RES = 0.05
BELOW, ABOVE, NAN_IS_SEED = 1, 2, 4
MODES = (BELOW, ABOVE, BELOW | NAN_IS_SEED, ABOVE | NAN_IS_SEED)
BATCH = 3
# rows x cols: 130 x 96 crosses the 64-row segments and a tile edge in both axes
SHAPES = [(1, 1), (5, 200), (70, 37), (130, 96), (257, 64)]
REACHES = [0, 1, 3, 9, 40]
ABOVE_THE_DIAGONAL = 400  # cells: more than the diagonal of every shape
REGION_SHAPE = (130, 96)
REGION_REACHES = [3, 9]
THRESHOLD = 0.5


def cap_for(cells, res=RES):
    """A max_distance whose reach is `cells` cells, away from both ties."""
    return (cells + 0.5) * res


def rects(rows, cols):
    """(row0, col0, h, w): the corners, the edges, single cells, the interior, the whole map."""
    return [(0, 0, 4, 5), (rows - 3, cols - 6, 3, 6), (0, cols - 2, 7, 2), (rows - 1, 0, 1, 9), (0, 30, 2, 11), (60, 0, 9, 1), (rows - 5, 40, 5, 3),
            (50, cols - 1, 20, 1), (64, 64, 1, 1), (0, 0, 1, 1), (61, 60, 8, 9), (17, 23, 40, 31), (0, 0, rows, cols)]


def maps(rows, cols, seed):
    """[BATCH] (rows, cols) layers in [0, 1] around the threshold: bag-like values with NaN speckle; the last map has no cell
    below the threshold (and none that is NaN): it is empty under BELOW."""
    rng = np.random.default_rng(seed)
    out = []
    for m in range(BATCH):
        a = M.values("bag", rng, rows, cols)
        a = (a * np.float32(1.6)).astype(np.float32)  # values on both sides of the threshold, some equal to no one's
        u = rng.random((rows, cols))
        a[u < 0.02] = np.float32(THRESHOLD)  # cells equal to the threshold: seeds in neither mode
        if m < BATCH - 1:
            a[rng.random((rows, cols)) < 0.03] = np.nan
            if m == 1:  # few seeds: long walks
                keep = rng.random((rows, cols)) < 0.01
                a[~keep & ~np.isnan(a)] = np.float32(THRESHOLD)
        else:
            a = np.maximum(a, np.float32(THRESHOLD))
        out.append(a)
    return out


# (rows, cols, reach in cells, TE_OPT_DISTANCE_ROUTE, the route claimed): 1 is tiled wherever 64 rows x (64 + 2 R) columns (or the map's,
# if fewer) of 2 bytes fit in 64 KiB, 2 the route of any reach always
def staged_bytes(cols, reach):
    return 64 * min(64 + 2 * reach, cols) * 2


ROUTE_CLAIMS = [(r_, c_, reach, opt, "tiled" if opt == 1 and staged_bytes(c_, reach) <= 64 * 1024 else "any")
                for (r_, c_) in SHAPES for reach in REACHES + [ABOVE_THE_DIAGONAL] for opt in (1, 2)]

# Tall maps, long halos and the LDS limit: shapes the sweep above cannot reach.  Every figure is a claim, written down from the
# plan as printed once and held to it by tests/test_distance_plan.py; None: not claimed.
#   rows, cols, reach, option, route, LDS bytes, seg_chunks, p1_segs                what the case is for
TALL_CASES = [
    (300, 8, 40, 0, "tiled", None, 4, 2),       # a second segment of 44 rows, the halo one chunk
    (520, 8, 9, 0, "tiled", None, 4, 3),        # three segments
    (577, 6, 100, 0, "any", 0, 8, 2),           # a pre-halo of two chunks before the second segment, empty chunks behind the first
    (577, 6, 100, 1, "tiled", 768, 8, 2),       # ... and the same g on the tiled route
    (800, 6, 150, 0, "any", 0, 12, 2),          # three chunks of halo either way
    (4100, 5, 1000, 0, "any", 0, 64, 2),        # seg_chunks == kMaxSegChunks: every lane holds a mask
    (4100, 5, 1000, 1, "tiled", 640, 64, 2),
    (3, 600, 224, 1, "tiled", 65536, None, None),   # 64 + 2 R = 512 staged columns: exactly the LDS limit
    (3, 600, 225, 1, "any", 0, None, None),         # ... one column more: the forced route falls back
    (3, 600, 224, 0, "any", 0, None, None),
    (70, 200, 64, 0, "tiled", 24576, None, None),   # route by plan at kTiledMaxReach
    (70, 200, 65, 0, "any", 0, None, None),         # ... and one cell above it
]
# the cases whose segments are claimed: tests/test_distance_ref.py shows on their inputs that the branch is reached
TALL_SEGMENTED = sorted({(r_, c_, reach, seg) for (r_, c_, reach, _o, _r, _l, seg, _n) in TALL_CASES if seg is not None})

LAYOUTS = 14


def layout_rows(k, rows, reach, b):
    """The rows of the seeds of layout k of a designed column; b: the first row of the second segment claimed (seg_chunks * 64).
    Positions outside the map are dropped."""
    pos = [[], [0], [rows - 1], [b - 1], [b], [b - reach], [b - reach - 1], [b + reach - 1], [b - 1 + reach], [b + reach], [b - 65, b + 64],
           range(63, rows, 64), range(0, rows, 64), range(rows)][k]
    return [r for r in pos if 0 <= r < rows]


def designed(rows, cols, reach, seg_chunks, mode):
    """Maps of designed columns for `mode`.  Free cells hold the threshold (a seed in neither mode); a seed holds a value on the
    mode's side of it, and under NAN_IS_SEED every other seed is a NaN instead, so the seeds are the same cells in every mode.
    First the maps whose column j carries layout j, taken in turn, as many maps as it takes for every layout to appear (the
    turn goes on from one map to the next and wraps).  Then one map per layout with that layout in the middle column alone:
    in maps this narrow a seed of any column lies within the reach of every other column, and only a column without
    neighbours shows all of its own column distances in the output."""
    seg = 1 if seg_chunks is None else seg_chunks
    value = np.float32(THRESHOLD - 0.4) if (mode & 3) == BELOW else np.float32(THRESHOLD + 0.4)

    def column(a, j, k):
        for r in layout_rows(k, rows, reach, seg * 64):
            a[r, j] = np.nan if (mode & NAN_IS_SEED) and (r + j) % 2 else value

    out = []
    for first in range(0, LAYOUTS, cols):
        a = np.full((rows, cols), np.float32(THRESHOLD), np.float32)
        for j in range(cols):
            column(a, j, (first + j) % LAYOUTS)
        out.append(a)
    for k in range(LAYOUTS):
        a = np.full((rows, cols), np.float32(THRESHOLD), np.float32)
        column(a, cols // 2, k)
        out.append(a)
    return out


def tall_batches(rows, cols, reach, seg_chunks, mode, seed):
    """The batches of BATCH maps of a tall case.  The first: designed columns, the few-seeds map, the map that is empty under
    BELOW; the others carry the remaining designed maps, the last one filled up with empty ones."""
    few, empty = maps(rows, cols, seed)[1:]
    d = designed(rows, cols, reach, seg_chunks, mode)
    rest = d[1:] + [empty] * (-(len(d) - 1) % BATCH)
    return [[d[0], few, empty]] + [rest[i:i + BATCH] for i in range(0, len(rest), BATCH)]


# Region form on a tall map.  (row0, col0, h, w) -> the claimed out (i0, j0, h, w), g.i0 and in.i0, where claimed
REGION_TALL = {
    "A": dict(shape=(577, 40), reach=100, seg_chunks=8,
              # seeds of map 0: 90 rows before the first rectangle's g (the first of its two chunks of pre-halo), one row outside
              # its `in`, 90 rows before the second rectangle's g, 90 rows behind the third's
              seeds=[(330, 12), (319, 30), (110, 25), (190, 3)],
              rects=[((520, 10, 3, 4), dict(out=(420, 0, 157, 40), g_i0=420, in_i0=320)),  # g.i0 no multiple of 64; two chunks of pre-halo, half masked
                     ((300, 0, 1, 1), dict(out=(200, 0, 201, 40))),
                     ((0, 0, 1, 1), {}),
                     ((576, 39, 1, 1), {}),
                     ((0, 0, 577, 40), dict(out=(0, 0, 577, 40), g_i0=0, in_i0=0))]),
    "B": dict(shape=(520, 8), reach=9, seg_chunks=4,
              # before g inside and outside `in`, before and behind the boundary of the region's two segments (row 347), behind g
              seeds=[(85, 1), (81, 6), (340, 6), (350, 0), (405, 7), (415, 1)],
              rects=[((100, 2, 300, 3), dict(out=(91, 0, 318, 8), g_i0=91, in_i0=82, plan_seg_chunks=4, p1_segs=2))]),  # rows [91, 409): two segments inside a region
}



def seeded(rows, cols, cells, mode):
    """A map of free cells with seeds at `cells`, valued as in designed()."""
    a = np.full((rows, cols), np.float32(THRESHOLD), np.float32)
    for n, (r, c) in enumerate(cells):
        a[r, c] = np.nan if (mode & NAN_IS_SEED) and n % 2 else np.float32(THRESHOLD - 0.4) if (mode & 3) == BELOW else np.float32(THRESHOLD + 0.4)
    return a


def region_base(name, mode):
    """[BATCH] maps a tall region case starts from: its seeds, the few-seeds map, the map that is empty under BELOW."""
    case = REGION_TALL[name]
    rows, cols = case["shape"]
    return [seeded(rows, cols, case["seeds"], mode)] + maps(rows, cols, 1000 * rows + cols)[1:]


# Values at the edges of the comparison (tests/test_gpu_distance.py::test_values_at_the_edges...): threshold -> the pool of cells
EDGE_SHAPE = (70, 37)
EDGE_REACH = 9
EDGE_RESOLUTIONS = [0.013, 0.1, 1.0, 0.0025]
_F = np.float32
EDGE_POOLS = [
    (0.0, _F([0.0, -0.0, 1e-45, -1e-45, 1.1754944e-38, -1.1754944e-38, np.inf, -np.inf, np.nan, 1.0, -1.0])),
    (-0.25, _F([-0.25, np.nextafter(_F(-0.25), _F(0)), np.nextafter(_F(-0.25), _F(-1)), 0.0, -0.0, -0.5, 1e-45, -1e-45, np.inf, -np.inf, np.nan])),
    (0.1, _F([_F(0.1), np.nextafter(_F(0.1), _F(0)), np.nextafter(_F(0.1), _F(1)), 0.0, 0.2, -1e-45, np.inf, -np.inf, np.nan])),  # 0.1: a double
]
TIE_CELLS = [1, 2, 5, 10]       # max_distance = k * res: d2 = k * k is on the cap
TIE_SQUARES = [2, 5, 8]         # max_distance = res * sqrt(k), in double: d2 = k is


def edge_maps(threshold, pool, mode, seed):
    """[BATCH] maps of EDGE_SHAPE: cells drawn from the pool; the same with about 1 % of its seeds kept and the others set to
    the threshold; and a map of cells equal to the threshold (for 0.0: of both zeros), which has no seed in any mode."""
    rows, cols = EDGE_SHAPE
    rng = np.random.default_rng(seed)
    a = pool[rng.integers(0, len(pool), (rows, cols))].astype(np.float32)
    t = np.float32(threshold)
    with np.errstate(invalid="ignore"):
        s = a < t if (mode & 3) == BELOW else a > t
    if mode & NAN_IS_SEED:
        s = s | np.isnan(a)
    b = a.copy()
    b[s & (rng.random((rows, cols)) >= 0.01)] = t
    c = np.full((rows, cols), t, np.float32)
    if t == 0:
        c[::2] = np.float32(-0.0)
    return [a, b, c]


def tie_maps(seed):
    """[BATCH] maps of EDGE_SHAPE: one seed at (30, 15), whose neighbours have every small d2; the few-seeds map; an empty map."""
    rows, cols = EDGE_SHAPE
    a = np.full((rows, cols), np.float32(THRESHOLD), np.float32)
    a[30, 15] = np.float32(0.1)
    return [a] + maps(rows, cols, seed)[1:]
