"""Shapes and inputs of the connected-region tests (te_run_components / te_run_reachable), seeded.  A case is a free mask; the
layer of a mode is made from it, so both comparison modes see the same regions.  tests/test_components_ref.py holds the designed
inputs to the counts stated here, tests/test_components_plan.py the shapes to the tile geometry claimed here."""
import numpy as np

BELOW, ABOVE, NAN_IS_SEED = 1, 2, 4
MODES = [BELOW, ABOVE]
CONNECTIVITIES = [4, 8]
THRESHOLD = 0.5
RES = 0.05

SHAPES = [(1, 1), (1, 9), (9, 1), (3, 3), (70, 70), (130, 67), (577, 6), (5, 300), (512, 384)]
# (rows, cols) -> the tiles along the rows and along the columns the device uses at least (tiles of 64 x 64 cells)
MULTI_TILE = {(70, 70): (2, 2), (130, 67): (3, 2), (577, 6): (10, 1), (5, 300): (1, 5), (512, 384): (8, 6)}
# shapes with a seam along both axes: the designed inputs cross both there
BOTH_SEAMS = [s for s, (a, b) in MULTI_TILE.items() if a >= 2 and b >= 2]
RANDOM_FREE = {"random30": 0.30, "random50": 0.50, "random593": 0.593, "random80": 0.80}


def checkerboard(rows, cols):
    i, j = np.indices((rows, cols))
    return (i + j) % 2 == 0


def diagonal(rows, cols):
    i, j = np.indices((rows, cols))
    return i == j


def spiral(rows, cols):
    """A corridor of width 1 wound inward from (0, 0), with walls of width 1: one component, every cell with at most two free
    4-neighbours."""
    f = np.zeros((rows, cols), bool)
    dirs = [(0, 1), (1, 0), (0, -1), (-1, 0)]

    def is_free(i, j):
        return 0 <= i < rows and 0 <= j < cols and f[i, j]

    i = j = d = 0
    f[0, 0] = True
    while True:
        for turn in (0, 1):
            di, dj = dirs[(d + turn) % 4]
            ni, nj = i + di, j + dj
            # the next cell exists, and neither the cell behind it nor the cells beside it are corridor already
            if (0 <= ni < rows and 0 <= nj < cols and not f[ni, nj] and not is_free(ni + di, nj + dj)
                    and not is_free(ni + dj, nj + di) and not is_free(ni - dj, nj - di)):
                d = (d + turn) % 4
                i, j = ni, nj
                f[i, j] = True
                break
        else:
            return f


def comb(rows, cols):
    """Teeth on every second column, joined by row 0: one component."""
    f = np.zeros((rows, cols), bool)
    f[0, :] = True
    f[:, ::2] = True
    return f


def two_combs(rows, cols):
    """Comb A hangs from row 0 (teeth on columns 0, 4, ...), comb B stands on the last row (teeth on columns 2, 6, ...); a stub of
    B at (rows - 2, 1) touches A's first tooth tip (rows - 3, 0) diagonally and nowhere else: 4 -> two components, 8 -> one."""
    assert rows >= 6 and cols >= 5
    f = np.zeros((rows, cols), bool)
    f[0, :] = True
    f[1:rows - 2, 0::4] = True
    f[rows - 1, :] = True
    f[2:rows - 1, 2::4] = True
    f[rows - 2, 1] = True
    return f


def masks(rows, cols, seed):
    """name -> (free mask, NaN mask or None).  With a NaN mask the case runs twice: the NaN cells free (no bit) and blocked."""
    rng = np.random.default_rng(seed)
    out = {"all_free": (np.ones((rows, cols), bool), None), "all_blocked": (np.zeros((rows, cols), bool), None),
           "checkerboard": (checkerboard(rows, cols), None), "diagonal": (diagonal(rows, cols), None),
           "spiral": (spiral(rows, cols), None), "comb": (comb(rows, cols), None)}
    if rows >= 6 and cols >= 5:
        out["two_combs"] = (two_combs(rows, cols), None)
    for name, p in RANDOM_FREE.items():
        out[name] = (rng.random((rows, cols)) < p, None)
    out["nan_speckle"] = (rng.random((rows, cols)) < 0.6, rng.random((rows, cols)) < 0.1)
    out["at_threshold"] = (rng.random((rows, cols)) < 0.4, None)
    return out


def layer_of(free, mode, seed, nan=None, at_threshold=False):
    """A float32 layer [rows, cols] whose free cells under (mode, THRESHOLD) are `free`; NaN where `nan` is set."""
    rng = np.random.default_rng(seed + 17)
    good = (0.55 + 0.4 * rng.random(free.shape)).astype(np.float32)
    bad = (0.05 + 0.4 * rng.random(free.shape)).astype(np.float32)
    if at_threshold:
        good[:] = np.float32(THRESHOLD)
    v = np.where(free, good, bad).astype(np.float32)
    if (mode & 3) == ABOVE:
        v = (np.float32(1.0) - v).astype(np.float32)
    if nan is not None:
        v[nan] = np.nan
    return v


def cases(rows, cols):
    """[(name, mode bits beside the comparison, free mask as the contract sees it, function mode -> layer)]"""
    seed = 1000 * rows + cols
    out = []
    for name, (free, nan) in masks(rows, cols, seed).items():
        if nan is None:
            out.append((name, 0, free, lambda mode, f=free, n=name: layer_of(f, mode, seed, None, n == "at_threshold")))
        else:
            out.append((name + "_free", 0, free | nan, lambda mode, f=free, m=nan: layer_of(f, mode, seed, m)))
            out.append((name + "_blocked", NAN_IS_SEED, free & ~nan, lambda mode, f=free, m=nan: layer_of(f, mode, seed, m)))
    return out


# ---- what only the device runs: the write pass beyond one turn, the starts kernel beyond its first lanes, unions that meet ----
# The write pass has at most 4096 workgroups of 256 threads: a map of more than WRITE_TURN cells makes some threads take a
# second turn.  BIG has 7,424 cells more (storage indices WRITE_TURN ...), BIG_THIN is 257 x 2 tiles for the batch form.
WRITE_TURN = 4096 * 256
BIG = (1100, 960)
BIG_THIN = (16400, 65)
ISLANDS_SHAPE = (130, 67)
PERFORATED_SHAPES = [(200, 200), (512, 384)]
SPLIT_ROW = 100
FLOAT_INEXACT = (4097, 4097)  # 2^24 + 8193 cells, odd: the smallest square whose cell count float32 cannot hold
MAX_STARTS = 256
B_FREE_POSITIONS = (63, 64, 127, 128, 191, 192, 255)  # list b of island_starts


def big_random(rows, cols, seed):
    """The free mask `random593` of a shape too large to build every mask of masks() for."""
    return np.random.default_rng(seed).random((rows, cols)) < RANDOM_FREE["random593"]


def islands(rows, cols):
    """Free 2 x 2 blocks at a pitch of 3 cells: block (a, b) is rows 3a .. 3a + 1, columns 3b .. 3b + 1 (whole blocks only).
    Every block is a component of 4 cells under both connectivities."""
    i, j = np.indices((rows, cols))
    return (i % 3 < 2) & (j % 3 < 2) & (i // 3 < island_grid(rows, cols)[0]) & (j // 3 < island_grid(rows, cols)[1])


def island_grid(rows, cols):
    """(blocks along the rows, along the columns) of islands(rows, cols)"""
    return (rows + 1) // 3, (cols + 1) // 3


def island_starts(rows, cols, seed):
    """Lists of MAX_STARTS starts on islands(rows, cols), from a seeded shuffle.  name -> (starts, islands hit):
    a  every start in an island of its own;
    b  positions 63, 64, 127, 128, 191, 192 and 255 (the last lane of a wavefront, the first of the next, the last start) on free
       cells of different islands, every other position on a blocked cell;
    c  the last start on a free cell, every other one on a blocked cell;
    d  128 islands, each hit twice (by different cells)."""
    rng = np.random.default_rng(seed)
    na, nb = island_grid(rows, cols)
    assert na * nb >= MAX_STARTS
    order = rng.permutation(na * nb)

    def cell(block, corner):
        return (3 * int(block // nb) + corner // 2, 3 * int(block % nb) + corner % 2)

    blocked = np.argwhere(~islands(rows, cols))
    walls = [tuple(int(v) for v in blocked[k]) for k in rng.permutation(len(blocked))[:MAX_STARTS]]
    a = [cell(order[k], int(rng.integers(4))) for k in range(MAX_STARTS)]
    b = list(walls)
    for n, k in enumerate(B_FREE_POSITIONS):
        b[k] = cell(order[300 + n], int(rng.integers(4)))
    c = list(walls)
    c[MAX_STARTS - 1] = cell(order[400], int(rng.integers(4)))
    corners = rng.permutation(4)
    d = [cell(order[500 + k % 128], int(corners[k // 128])) for k in rng.permutation(MAX_STARTS)]
    return {"a": (a, MAX_STARTS), "b": (b, len(B_FREE_POSITIONS)), "c": (c, 1), "d": (d, 128)}



def perforated(rows, cols, split=False):
    """All free, except every second cell of every seam column (i odd, j = 64, 128, ...) and of every seam row (i = 64, 128, ...,
    j odd).  A free seam cell then has a blocked cell before it along its seam, so the seam pass can save no union: every free
    seam cell of a tile edge unites the same two tile-local components, about 32 threads on the same two roots at once.  One
    component under both connectivities; split: row SPLIT_ROW is blocked as well, two components of different sizes."""
    i, j = np.indices((rows, cols))
    f = ~(((i % 2 == 1) & (j % 64 == 0) & (j >= 64)) | ((i % 64 == 0) & (i >= 64) & (j % 2 == 1)))
    if split:
        f[SPLIT_ROW, :] = False
    return f


def rake(rows, cols):
    """A hub on every column seam: the seam column (j = 64, 128, ...) is free over all rows, and every even row is free over the 32
    columns before it.  The teeth of a tile meet nowhere but in the seam column, so the seam pass unites 32 tile-local components
    with smaller roots to the one root of the seam column's piece: 32 threads lower the same entry to different values, and a
    union dropped on the way (the retry of `unite`) leaves a tooth outside.  Components: one per seam column, of
    rows + 32 * ceil(rows / 2) cells, and the teeth behind the last seam column alone."""
    i, j = np.indices((rows, cols))
    return ((j % 64 == 0) & (j >= 64)) | ((i % 2 == 0) & (j % 64 >= 32))


def start_sets(lab, free):
    """The start lists of a case: one in the largest component; one on a blocked cell; two in different components; one start
    repeated; the map's four corners.  Lists that the map cannot supply are left out."""
    rows, cols = lab.shape
    sets = {"corners": [(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1)]}
    live = lab[lab >= 0]
    if live.size:
        ids, counts = np.unique(live, return_counts=True)
        big = int(ids[np.argmax(counts)])
        first = (big % rows, big // rows)
        sets["largest"] = [first]
        sets["repeated"] = [first, first, first]
        if ids.size > 1:
            other = int(ids[ids != big][-1])
            sets["two"] = [first, (other % rows, other // rows)]
    blocked = np.argwhere(~free)
    if blocked.size:
        sets["blocked"] = [tuple(int(v) for v in blocked[len(blocked) // 2])]
    return sets
