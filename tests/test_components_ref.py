"""The definition of the connected regions (tests/ref_py/components_ref.py) held to itself: the counts of the designed inputs of
tests/components_cases.py, scipy.ndimage.label up to renaming, the two connectivities differing exactly where designed, the
axes swapped, and the free cells of the contract (the threshold itself, NaN with and without the bit); and the inputs designed for the paths only the
device runs (islands and their start lists, perforated) are what tests/test_gpu_components.py takes them for."""
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


def test_islands_are_946_components_of_4_cells():
    rows, cols = K.ISLANDS_SHAPE
    f = K.islands(rows, cols)
    assert K.island_grid(rows, cols) == (43, 22)
    for conn in (4, 8):
        lab = R.labels(f, conn)
        assert R.stats_of(lab) == (946, 4 * 946, 4, 0)
        assert set(np.unique(R.sizes_of(lab))) == {0.0, 4.0}


def test_island_start_lists_hit_the_islands_they_claim():
    rows, cols = K.ISLANDS_SHAPE
    f = K.islands(rows, cols)
    lists = K.island_starts(rows, cols, 5)
    assert {k: n for k, (_s, n) in lists.items()} == {"a": 256, "b": 7, "c": 1, "d": 128}
    for conn in (4, 8):
        lab = R.labels(f, conn)
        for name, (starts, n) in lists.items():
            assert len(starts) == K.MAX_STARTS
            hit = [int(lab[r, c]) for r, c in starts if lab[r, c] >= 0]
            assert len(set(hit)) == n, name
            assert R.stats_of(lab, starts) == (946, 4 * 946, 4, 4 * n), name
        assert len([1 for r, c in lists["a"][0] if f[r, c]]) == 256
        # b: exactly the seven positions are free, and each of them alone carries an island
        b = lists["b"][0]
        assert tuple(k for k, (r, c) in enumerate(b) if f[r, c]) == K.B_FREE_POSITIONS == (63, 64, 127, 128, 191, 192, 255)
        whole = R.reachable_of(lab, b)
        for k in K.B_FREE_POSITIONS:
            assert not np.array_equal(R.reachable_of(lab, b[:k] + b[k + 1:]), whole), k
        c = lists["c"][0]
        assert [k for k, (r, c_) in enumerate(c) if f[r, c_]] == [255]
        # d: every island hit is hit twice, by two different cells
        d = lists["d"][0]
        assert len(set(d)) == 256 and sorted(np.unique([int(lab[r, c_]) for r, c_ in d], return_counts=True)[1].tolist()) == [2] * 128
    # seeded: the same lists again
    assert K.island_starts(rows, cols, 5) == lists


@pytest.mark.parametrize("rows,cols", K.PERFORATED_SHAPES)
def test_perforated_is_one_component_but_for_the_tile_corners(rows, cols):
    """A corner cell (64a, 64b) is free and all four of its straight neighbours are blocked, so under connectivity 4 it is a
    component of its own; every other free cell is in the one large component.  Under connectivity 8 all is one component."""
    f = K.perforated(rows, cols)
    corners = ((rows - 1) // 64) * ((cols - 1) // 64)
    blocked = sum(len(range(1, rows, 2)) for _ in range(64, cols, 64)) + sum(len(range(1, cols, 2)) for _ in range(64, rows, 64))
    nfree = rows * cols - blocked
    assert int(f.sum()) == nfree
    assert R.stats_of(R.labels(f, 8)) == (1, nfree, nfree, 0)
    lab = R.labels(f, 4)
    assert R.stats_of(lab) == (1 + corners, nfree, nfree - corners, 0)
    assert (R.sizes_of(lab)[64:rows:64, 64:cols:64] == 1.0).all() and int((R.sizes_of(lab) == 1.0).sum()) == corners


@pytest.mark.parametrize("rows,cols", K.PERFORATED_SHAPES)
def test_perforated_split_has_two_components_of_different_sizes(rows, cols):
    f = K.perforated(rows, cols, split=True)
    assert not f[K.SPLIT_ROW].any() and np.array_equal(np.delete(f, K.SPLIT_ROW, 0), np.delete(K.perforated(rows, cols), K.SPLIT_ROW, 0))
    corners = ((rows - 1) // 64) * ((cols - 1) // 64)
    lab = R.labels(f, 8)
    ids, counts = np.unique(lab[lab >= 0], return_counts=True)
    assert len(ids) == 2 and counts[0] != counts[1] and lab[0, 0] != lab[rows - 1, cols - 1]
    assert (lab[:K.SPLIT_ROW][f[:K.SPLIT_ROW]] == lab[0, 0]).all() and (lab[K.SPLIT_ROW + 1:][f[K.SPLIT_ROW + 1:]] == lab[rows - 1, cols - 1]).all()
    lab = R.labels(f, 4)
    ids, counts = np.unique(lab[lab >= 0], return_counts=True)
    large = sorted(counts[counts > 1].tolist())
    assert len(ids) == 2 + corners and len(large) == 2 and large[0] != large[1] and lab[0, 0] != lab[rows - 1, cols - 1]


@pytest.mark.parametrize("rows,cols", K.PERFORATED_SHAPES)
def test_rake_is_one_component_per_seam_column_held_together_by_that_column_alone(rows, cols):
    f = K.rake(rows, cols)
    seams = list(range(64, cols, 64))
    loose = len(range(0, rows, 2)) if cols - seams[-1] > 32 else 0  # teeth behind the last seam column
    for conn in (4, 8):
        lab = R.labels(f, conn)
        size = R.sizes_of(lab)
        assert R.stats_of(lab)[0] == len(seams) + loose and R.stats_of(lab)[2] == rows + 32 * len(range(0, rows, 2))
        for j in seams:
            assert (lab[:, j] == lab[0, j]).all() and (lab[0::2, j - 32:j] == lab[0, j]).all() and size[0, j] == rows + 32 * len(range(0, rows, 2))
            # without the seam column every tooth is alone: no union of the seam pass is implied by the others
            g = f.copy()
            g[:, j] = False
            assert (R.sizes_of(R.labels(g, conn))[0::2, j - 32:j] == 32.0).all()
