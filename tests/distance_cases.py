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
