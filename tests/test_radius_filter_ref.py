"""tests/ref_py/radius_filter_ref.py (the yardstick of tests/test_gpu_radius_filter.py, vectorised over the centres) against the contract
written literally: one GridMapRef.circle walk per centre, a double sum in iterator order.  Bit patterns throughout."""
import numpy as np
import pytest

from tests import median_fill_cases as M
from tests import radius_filter_cases as K
from tests.ref_py import radius_filter_ref as R
from tests.ref_py.grid_map_ref import GridMapRef

POS = (0.0123, -0.0371)  # no multiple of the resolution
# radius 0, below one cell, 1.5 and 3.5 cells, the whole-cell tie radii, larger than the map
CELLS = [0.0, 0.5, 1.5, 3.5, 3, 5, 40.0]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("cells", CELLS)
@pytest.mark.parametrize("rows,cols", [(12, 9), (20, 17)])
def test_vectorised_equals_the_literal_loop(rows, cols, cells):
    gm = GridMapRef(rows, cols, K.RES, POS)
    rng = np.random.default_rng(rows * 100 + int(cells * 2))
    for values, holes in (("bag", "speckle_5"), ("cancel", "none"), ("mixed_signs", "inf_cells"), ("scales", "block_30"), ("bag", "all_nan")):
        a = M.punch(holes, rng, K.values(values, rng, rows, cols))
        for op in K.OPS:
            got = R.radius_filter(a, gm, K.radius_of(cells), op)
            want = R.radius_filter_loop(a, gm, K.radius_of(cells), op)
            assert np.array_equal(bits(got), bits(want)), (values, holes, op, np.argwhere(bits(got) != bits(want))[:6])


def test_the_tie_radii_have_cells_on_the_circle_that_centres_decide_differently():
    """What makes the per-centre decision matter: at 3 cells, off the grid, the cell three rows up is inside for some centres only."""
    gm = GridMapRef(20, 17, K.RES, POS)
    inside = set()
    for i in range(3, 20):
        inside.add((i - 3, 8) in set(gm.circle(gm.position((i, 8)), K.radius_of(3))))
    assert inside == {True, False}


def test_radius_zero_is_the_centre_and_minus_zero_sums_to_plus_zero():
    gm = GridMapRef(12, 9, K.RES, POS)
    a = np.full((12, 9), -0.0, np.float32)
    a[3, 3] = np.inf
    mean0 = R.radius_filter(a, gm, 0.0, K.MEAN)
    assert np.isnan(mean0[3, 3]) and bits(mean0).ravel()[0] == 0  # (double)(-0.0) added to +0.0 is +0.0
    assert bits(R.radius_filter(a, gm, K.radius_of(1.5), K.MEAN))[0, 0] == 0
    assert bits(R.radius_filter(a, gm, K.radius_of(1.5), K.MIN))[0, 0] == 0x80000000
    b = np.zeros((12, 9), np.float32)
    b[5, 5] = -0.0
    assert bits(R.radius_filter(b, gm, K.radius_of(1.5), K.MIN))[5, 4] == 0x80000000  # -0.0 sorts below +0.0
