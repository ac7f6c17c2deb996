"""tests/ref_py/distance_ref.py -- the definition of te_run_distance as a brute-force loop -- held to vectors computed by hand; and the
inputs of the tall and the edge cases of tests/distance_cases.py held, by that definition alone, to what they are named for."""
import numpy as np
import pytest

from tests import distance_cases as K
from tests.ref_py import distance_ref as D

RES = 0.05


def f32(x):
    return np.float32(x)


def test_single_seed_and_the_3_4_5_cell():
    a = np.ones((9, 8), np.float32)
    a[2, 1] = 0.0
    d = D.distance(a, D.BELOW, 0.5, 10.0, RES)
    assert d[2, 1] == 0.0 and d.dtype == np.float32
    assert d[5, 5] == f32(5 * RES) and d[6, 4] == f32(5 * RES)  # 3-4-5 and 4-3-5: exactly 5 cells
    assert d[2, 2] == f32(RES) and d[3, 2] == f32(np.sqrt(2.0) * RES) and d[8, 7] == f32(np.sqrt(72.0) * RES)
    for i in range(9):
        for j in range(8):
            assert d[i, j] == f32(np.sqrt(float((i - 2) ** 2 + (j - 1) ** 2)) * RES)


def test_two_seeds_at_equal_d2():
    a = np.ones((5, 7), np.float32)
    a[2, 0] = a[2, 6] = -1.0
    d = D.distance(a, D.BELOW, 0.0, 10.0, RES)
    assert d[2, 3] == f32(3 * RES) and d[0, 3] == f32(np.sqrt(13.0) * RES)
    assert np.array_equal(d, d[:, ::-1]) and np.array_equal(d, d[::-1, :])


def test_no_seed_and_all_seeds():
    a = np.ones((4, 6), np.float32)
    d = D.distance(a, D.BELOW, 0.5, 0.37, RES)
    assert (d == f32(0.37)).all()
    z = D.distance(a, D.ABOVE, 0.5, 0.37, RES)
    assert (z == 0.0).all() and not np.signbit(z).any()


def test_nan_cells_with_and_without_the_flag():
    a = np.ones((3, 6), np.float32)
    a[1, 1] = np.nan
    a[1, 4] = 0.0
    plain = D.distance(a, D.BELOW, 0.5, 10.0, RES)
    assert plain[1, 1] == f32(3 * RES) and plain[1, 0] == f32(4 * RES)  # the NaN cell is an ordinary cell
    flag = D.distance(a, D.BELOW | D.NAN_IS_SEED, 0.5, 10.0, RES)
    assert flag[1, 1] == 0.0 and flag[1, 0] == f32(RES) and flag[1, 4] == 0.0
    assert not np.isnan(plain).any() and not np.isnan(flag).any()
    # ABOVE: a NaN is no seed without the flag either
    assert (D.distance(np.full((2, 2), np.nan, np.float32), D.ABOVE, 0.0, 1.0, RES) == f32(1.0)).all()
    assert (D.distance(np.full((2, 2), np.nan, np.float32), D.ABOVE | D.NAN_IS_SEED, 0.0, 1.0, RES) == 0.0).all()


def test_a_value_equal_to_the_threshold_is_no_seed_in_either_mode():
    a = np.full((3, 3), 0.5, np.float32)
    assert not D.seeds(a, D.BELOW, 0.5).any() and not D.seeds(a, D.ABOVE, 0.5).any()
    # the threshold is compared as a float: 0.1 (double) rounds to the float the cell holds
    b = np.full((2, 2), np.float32(0.1), np.float32)
    assert not D.seeds(b, D.BELOW, 0.1).any() and not D.seeds(b, D.ABOVE, 0.1).any()
    assert D.seeds(np.float32([[0.25]]), D.BELOW, 0.5).all() and D.seeds(np.float32([[0.75]]), D.ABOVE, 0.5).all()


def cap2_by_loop(max_distance, res):
    q, r2 = max_distance * max_distance, res * res
    k = 0
    while float(k + 1) * r2 <= q:
        k += 1
    return k


def test_cap_ties():
    for md, res in [(0.5, 0.05), (0.15, 0.03), (2.0, 0.05), (10.0, 0.05), (0.37, 0.05), (1e-9, 0.05), (3.0, 1.0), (5.0, 1.0)]:
        cap2, R = D.cap_cells(md, res)
        assert cap2 == cap2_by_loop(md, res), (md, res)
        assert R * R <= cap2 < (R + 1) * (R + 1)
    # what the doubles make of the two ties: 0.5 m is 10 cells of 0.05 m only if 100 * (0.05 * 0.05) <= 0.25 holds as rounded
    assert D.cap_cells(0.5, 0.05) == ((100, 10) if 100.0 * (0.05 * 0.05) <= 0.5 * 0.5 else (99, 9))
    assert D.cap_cells(0.15, 0.03) == ((25, 5) if 25.0 * (0.03 * 0.03) <= 0.15 * 0.15 else (24, 4))
    assert D.cap_cells(3.0, 1.0) == (9, 3) and D.cap_cells(1e-9, 0.05) == (0, 0)


def test_the_cap_cuts_at_cap2():
    a = np.ones((1, 12), np.float32)
    a[0, 0] = 0.0
    cap2, R = D.cap_cells(0.2, RES)
    d = D.distance(a, D.BELOW, 0.5, 0.2, RES)
    for j in range(12):
        assert d[0, j] == (f32(np.sqrt(float(j * j)) * RES) if j * j <= cap2 else f32(0.2)), j
    assert d[0, R] == f32(float(R) * RES) and d[0, R + 1] == f32(0.2)
    # R = 0: only the seeds themselves are within the cap
    e = D.distance(a, D.BELOW, 0.5, 0.01, RES)
    assert e[0, 0] == 0.0 and (e[0, 1:] == f32(0.01)).all()


# --- the inputs of the tall cases of tests/distance_cases.py reach the branches they are named for (no GPU, nothing of csrc/) ---

def column_nearest_rows(seed):
    """Per cell of a [rows, cols] seed array: the distance along its column to the nearest seed before (or at) it and behind (or at)
    it, and those seeds' rows; no seed: distance a large number."""
    rows, cols = seed.shape
    big = 1 << 40
    idx = np.arange(rows)[:, None]
    last = np.maximum.accumulate(np.where(seed, idx, -big), axis=0)
    nxt = np.minimum.accumulate(np.where(seed, idx, big)[::-1], axis=0)[::-1]
    return idx - last, last, nxt - idx, nxt


def tall_inputs(rows, cols, reach, seg_chunks):
    out = []
    for a in K.designed(rows, cols, reach, seg_chunks, K.BELOW):
        seed = D.seeds(a, K.BELOW, K.THRESHOLD)
        out.append((seed, D.squared_cells(seed.T).T))  # (the definition is symmetric: the short axis goes first)
    return out


@pytest.mark.parametrize("rows,cols,reach,seg_chunks", K.TALL_SEGMENTED)
def test_tall_inputs_reach_the_branches_they_are_named_for(rows, cols, reach, seg_chunks):
    """Conditions on the inputs alone.  Each one asks for a cell whose column distance is also its distance in the map (d2 of the
    definition equals it squared), so that the output shows what pass 1 made of it."""
    b = seg_chunks * 64
    assert rows > b
    before_far = behind_far = at_reach = past_reach = saturated = False
    seg = (np.arange(rows) // b)[:, None]
    for seed, d2 in tall_inputs(rows, cols, reach, seg_chunks):
        up, up_row, down, down_row = column_nearest_rows(seed)
        col = np.minimum(up, down)
        shows = col.astype(np.int64) ** 2 == d2
        # the nearest seed of the column lies in an earlier / a later segment, more than a chunk away and within the reach
        before_far |= bool((shows & (seg > 0) & (up < down) & (up_row // b < seg) & (up > 64) & (up <= reach)).any())
        behind_far |= bool((shows & (down < up) & (down_row // b > seg) & (down > 64) & (down <= reach)).any())
        at_reach |= bool((shows & (col == reach)).any())
        past_reach |= bool((shows & (col == reach + 1)).any())
        saturated |= bool((col > reach).all(axis=0).any())
    if reach > 64:
        assert before_far and behind_far
    assert at_reach and past_reach and saturated
    # the modes share their seeds: the NaN cells of the NAN_IS_SEED maps are the seeds the other maps hold as values
    for mode in K.MODES:
        for a, z in zip(K.designed(rows, cols, reach, seg_chunks, mode), K.designed(rows, cols, reach, seg_chunks, K.BELOW)):
            assert np.array_equal(D.seeds(a, mode, K.THRESHOLD), D.seeds(z, K.BELOW, K.THRESHOLD))
            assert mode & K.NAN_IS_SEED or not np.isnan(a).any()
        if mode & K.NAN_IS_SEED:  # (the first map: some seeds are NaN cells, some are values)
            assert np.isnan(a0 := K.designed(rows, cols, reach, seg_chunks, mode)[0]).any() and D.seeds(a0, mode & 3, K.THRESHOLD).any()


def test_edge_inputs_hold_what_they_are_named_for():
    zero = dict((float(t), p) for t, p in K.EDGE_POOLS)[0.0]
    assert not D.seeds(np.float32([[-0.0, 0.0]]), D.BELOW, 0.0).any() and not D.seeds(np.float32([[-0.0, 0.0]]), D.ABOVE, 0.0).any()
    tiny = zero[(zero != 0) & (np.abs(zero) < np.float32(1.1754944e-38))]
    assert len(tiny) == 2 and D.seeds(tiny[None, :], D.BELOW, 0.0).sum() == 1 and D.seeds(tiny[None, :], D.ABOVE, 0.0).sum() == 1
    near = dict((float(t), p) for t, p in K.EDGE_POOLS)[0.1]
    assert D.seeds(near[None, :3], D.BELOW, 0.1).tolist() == [[False, True, False]] and D.seeds(near[None, :3], D.ABOVE, 0.1).tolist() == [[False, False, True]]
    for threshold, pool in K.EDGE_POOLS:
        for mode in K.MODES:
            a, few, none = K.edge_maps(threshold, pool, mode, 7)
            assert 0 < D.seeds(few, mode, threshold).sum() < D.seeds(a, mode, threshold).sum() / 20 and not D.seeds(none, mode, threshold).any()
    # the ties: some cell of the single-seed map has d2 exactly k * k, and exactly k
    d2 = D.squared_cells(D.seeds(K.tie_maps(3)[0], D.BELOW, K.THRESHOLD))
    assert all((d2 == k * k).any() for k in K.TIE_CELLS) and all((d2 == k).any() for k in K.TIE_SQUARES)


def test_the_tall_region_case_reads_a_seed_two_chunks_before_its_g():
    """Case A, first rectangle, whatever the rectangle itself holds (here: all seeds): some cell of `out` has its nearest seed of
    the map in its own column, before g, in the first of the two chunks of pre-halo and inside `in`."""
    case = K.REGION_TALL["A"]
    (rows, cols), reach = case["shape"], case["reach"]
    (r0, c0, h, w), claim = case["rects"][0]
    a = K.region_base("A", K.BELOW)[0]
    a[r0:r0 + h, c0:c0 + w] = 0.0
    seed = D.seeds(a, K.BELOW, K.THRESHOLD)
    d2 = D.squared_cells(seed.T).T
    up, up_row, _down, _down_row = column_nearest_rows(seed)
    g0, in0 = claim["g_i0"], claim["in_i0"]
    i = np.arange(rows)[:, None]
    assert ((i >= g0) & (up_row >= in0) & (up_row < g0 - 64) & (up <= reach) & (up.astype(np.int64) ** 2 == d2)).any()
    assert seed[in0 - 1].any()  # and a seed lies one row outside `in`
