"""The shapes, radii and inputs of tests/test_gpu_radius_filter.py, kept apart from it so that tests/test_radius_plan.py can check --
without a GPU -- that every case lands on the kernel its GPU test claims.  Hole patterns and the other value kinds:
tests/median_fill_cases.py.  No Min fixture holds -0.0."""
import numpy as np

from tests import median_fill_cases as M

RES = M.RES
MEAN, MIN = 1, 2
OPS = (MEAN, MIN)
# (rows, cols, batch)
SHAPES = M.SHAPES
RADII_CELLS = [0.0, 0.5, 1.5, 3.5, 7.5]
TIE_CELLS = [3, 5]            # whole-cell radii: cells on the circle, decided per centre
OFF_GRID = (0.0123, -0.0371)  # a map position that is no multiple of the resolution
VALUE_RADII_CELLS = [1.5, 3.5]
BIG_WINDOW = (96, 80, 1, 40.0)
BLOCK_ROUTING = (130, 33, 1)
BLOCK_ROUTING_SEED = 71
VALUE_SHAPES = [(70, 37), (40, 21)]
VALUE_HOLES = ["none", "speckle_5", "inf_cells"]
# value kinds whose every workgroup passes the predicate at the radii above / none of whose workgroups does
PROVABLE_KINDS = ["bag", "mixed_signs", "negatives", "denormals"]
UNPROVABLE_KINDS = ["scales", "cancel"]
VALUE_KINDS = ["mixed_signs", "negatives", "denormals", "scales", "cancel"]

# (op, rows, cols, radius in cells, TE_OPT_RADIUS_ROUTE, the kernel claimed)
ROUTE_CLAIMS = [(op, r_, c_, rad, opt, "gather" if opt == 2 else "slide")
                for op in OPS for (r_, c_, _b) in SHAPES for rad in RADII_CELLS + TIE_CELLS for opt in (0, 1, 2)] + \
               [(op, BIG_WINDOW[0], BIG_WINDOW[1], BIG_WINDOW[3], opt, "gather" if opt == 2 else "slide") for op in OPS for opt in (0, 1, 2)]


def radius_of(cells, res=RES):
    return cells * res


def values(kind, rng, rows, cols):
    if kind == "cancel":  # huge values of both signs that cancel: the order of a sum decides what is left of the small ones
        a = rng.uniform(0.5, 2.0, (rows, cols)).astype(np.float32)
        u = rng.random((rows, cols))
        a[u < 0.15] = np.float32(2.0 ** 60)
        a[(u >= 0.15) & (u < 0.30)] = np.float32(-(2.0 ** 60))
        return a
    return M.values(kind, rng, rows, cols)


def block_routing_map(rng):
    """`bag` with `cancel` values in rows < 12, cols < 10 only."""
    rows, cols, _ = BLOCK_ROUTING
    a = M.values("bag", rng, rows, cols)
    a[:12, :10] = values("cancel", rng, rows, cols)[:12, :10]
    return a


def value_seed(rows, cells):
    return 17 + int(cells) + rows


def holey_maps(rows, cols, batch, seed, kinds, kind="bag"):
    """[batch] maps of value kind `kind`, map m with the hole pattern kinds[m % len(kinds)]."""
    rng = np.random.default_rng(seed)
    maps = [M.punch(kinds[m % len(kinds)], rng, values(kind, rng, rows, cols)) for m in range(batch)]
    assert not any(np.any(np.signbit(m) & (m == 0)) for m in maps)  # no Min fixture holds -0.0
    return maps
