"""The definition of the connected regions (tests/ref_py/components_ref.py) held to itself: the counts of the designed inputs of
tests/components_cases.py, scipy.ndimage.label up to renaming, the two connectivities differing exactly where designed, the
axes swapped, and the free cells of the contract (the threshold itself, NaN with and without the bit)."""
import numpy as np
import pytest

from tests import components_cases as K
from tests.ref_py import components_ref as R
from tests.ref_py import distance_ref as D

SMALL = [s for s in K.SHAPES if s[0] * s[1] <= 130 * 67]


def count(free, conn):
    return R.stats_of(R.labels(free, conn))[0]


@pytest.mark.parametrize("rows,cols", SMALL)
def test_designed_inputs_have_the_stated_counts(rows, cols):
    m = {k: v[0] for k, v in K.masks(rows, cols, 7).items()}
    n = rows * cols
    assert R.stats_of(R.labels(m["all_free"], 4)) == (1, n, n, 0) == R.stats_of(R.labels(m["all_free"], 8))
    assert R.stats_of(R.labels(m["all_blocked"], 4)) == (0, 0, 0, 0)
    # checkerboard: 4 -> every free cell alone; 8 -> one component (a map of one row or column has no diagonal step)
    nfree = int(m["checkerboard"].sum())
    assert R.stats_of(R.labels(m["checkerboard"], 4)) == (nfree, nfree, 1, 0)
    assert count(m["checkerboard"], 8) == (1 if min(rows, cols) > 1 else nfree)
    # a single diagonal
    d = min(rows, cols)
    assert int(m["diagonal"].sum()) == d and count(m["diagonal"], 4) == d and count(m["diagonal"], 8) == 1
    # the spiral: one corridor of width 1
    sp = m["spiral"]
    assert count(sp, 4) == 1 == count(sp, 8)
    pad = np.pad(sp, 1)
    around = pad[:-2, 1:-1].astype(int) + pad[2:, 1:-1] + pad[1:-1, :-2] + pad[1:-1, 2:]
    assert around[sp].max() <= 2 and (rows * cols < 9 or sp.sum() >= n // 3)
    assert count(m["comb"], 4) == 1 == count(m["comb"], 8)
    if "two_combs" in m:
        assert count(m["two_combs"], 4) == 2 and count(m["two_combs"], 8) == 1
    else:
        assert rows < 6 or cols < 5


@pytest.mark.parametrize("rows,cols", SMALL)
def test_labels_are_scipy_s_up_to_renaming(rows, cols):
    ndimage = pytest.importorskip("scipy.ndimage")
    for name, (free, _nan) in K.masks(rows, cols, 11).items():
        for conn in (4, 8):
            lab = R.labels(free, conn)
            theirs, n = ndimage.label(free, structure=np.ones((3, 3)) if conn == 8 else None)
            assert R.stats_of(lab)[0] == n, name
            assert ((lab >= 0) == (theirs > 0)).all()
            pairs = np.unique(np.stack([lab[free], theirs[free]]), axis=1)
            assert pairs.shape[1] == n and np.unique(pairs[0]).size == n and np.unique(pairs[1]).size == n, name
            # a label is the smallest storage index of its component
            idx = (np.arange(cols)[None, :] * rows + np.arange(rows)[:, None])
            for k in np.unique(lab[free])[:50]:
                assert idx[lab == k].min() == k


def test_connectivities_differ_exactly_where_designed():
    free = np.array([[1, 0, 0, 1], [0, 1, 0, 1], [0, 0, 0, 0], [1, 1, 0, 1]], bool)
    assert count(free, 4) == 5 and count(free, 8) == 4
    a, b = R.labels(free, 4), R.labels(free, 8)
    assert a[0, 0] != a[1, 1] and b[0, 0] == b[1, 1]
    assert (a[[0, 1], [3, 3]] == a[0, 3]).all() and (a[3, :2] == a[3, 0]).all() and a[3, 3] != a[0, 3]
    # a diagonal step connects whatever the two cells beside it are
    assert count(np.array([[1, 0], [0, 1]], bool), 8) == 1 and count(np.array([[1, 0], [0, 1]], bool), 4) == 2


def test_the_axes_can_be_swapped():
    for name, (free, _nan) in K.masks(70, 31, 3).items():
        for conn in (4, 8):
            assert np.array_equal(R.sizes_of(R.labels(free, conn)), R.sizes_of(R.labels(free.T.copy(), conn)).T), name


def test_free_cells_are_the_cells_te_run_distance_does_not_seed():
    v = np.array([[0.5, 0.25, 0.75, np.nan, -np.inf, np.inf]], np.float32)
    for mode in (R.BELOW, R.ABOVE, R.BELOW | R.NAN_IS_SEED, R.ABOVE | R.NAN_IS_SEED):
        assert np.array_equal(R.free(v, mode, 0.5), ~D.seeds(v, mode, 0.5))
    assert R.free(v, R.BELOW, 0.5).tolist() == [[True, False, True, True, False, True]]
    assert R.free(v, R.ABOVE | R.NAN_IS_SEED, 0.5).tolist() == [[True, True, False, False, True, False]]
    # every layer of the cases has the free cells it claims, in both modes
    for rows, cols in ((9, 1), (70, 70)):
        for name, extra, free, layer in K.cases(rows, cols):
            for mode in K.MODES:
                assert np.array_equal(R.free(layer(mode), mode | extra, K.THRESHOLD), free), (name, mode)
    at = [c for c in K.cases(70, 70) if c[0] == "at_threshold"][0]
    assert (at[3](K.BELOW)[at[2]] == np.float32(K.THRESHOLD)).all() and (at[3](K.ABOVE)[at[2]] == np.float32(K.THRESHOLD)).all()


def test_sizes_reachable_and_stats():
    free = np.array([[1, 1, 0, 1], [0, 0, 0, 1], [1, 0, 1, 0]], bool)
    v = np.where(free, 1.0, 0.0).astype(np.float32)
    assert R.sizes(v, R.BELOW, 0.5, 4).tolist() == [[2, 2, 0, 2], [0, 0, 0, 2], [1, 0, 1, 0]]
    assert R.sizes(v, R.BELOW, 0.5, 8).tolist() == [[2, 2, 0, 3], [0, 0, 0, 3], [1, 0, 3, 0]]
    assert R.reachable(v, R.BELOW, 0.5, 8, [(2, 2)]).tolist() == [[0, 0, 0, 1], [0, 0, 0, 1], [0, 0, 1, 0]]
    assert R.reachable(v, R.BELOW, 0.5, 4, [(1, 1)]).sum() == 0  # a start on a blocked cell reaches nothing
    assert R.stats(v, R.BELOW, 0.5, 4) == (4, 6, 2, 0) and R.stats(v, R.BELOW, 0.5, 8, [(0, 0), (0, 1), (2, 0)]) == (3, 6, 3, 3)
    assert R.sizes_of(R.labels(free, 4)).dtype == np.float32
