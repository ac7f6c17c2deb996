"""tests/ref_py/distance_ref.py -- the definition of te_run_distance as a brute-force loop -- held to vectors computed by hand."""
import numpy as np

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
