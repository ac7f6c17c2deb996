"""tests/ref_py/window_expression_ref.py, the yardstick of te_run_window_expression, against vectors worked out by hand from the
contract of include/travgpu.h: a 4 x 5 map with a NaN cell under all four edge handlings and both compute_empty_cells values,
rule 2 on window_length, and a window whose row-major double sum gives other bits than the contract's column order."""
import numpy as np
import pytest

from tests.ref_py import window_expression_ref as R

NAN = np.nan
A = np.array([[1, 2, 3, 4, 5],
              [6, 7, NAN, 9, 10],
              [11, 12, 13, 14, 15],
              [16, 17, 18, 19, 20]], np.float32)
X = "elevation"


def same(got, want):
    want = np.asarray(want, np.float32)
    return got.dtype == np.float32 and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])


def test_inside_visits_only_cells_with_a_whole_window():
    got = R.window_expression(A, f"meanOfFinites({X})", X, 3, "inside")
    assert same(got, [[NAN] * 5,
                      [NAN, 55 / 8, 64 / 8, 73 / 8, NAN],
                      [NAN, 100 / 8, 109 / 8, 118 / 8, NAN],
                      [NAN] * 5])
    # the NaN centre is not visited without compute_empty_cells
    got = R.window_expression(A, f"meanOfFinites({X})", X, 3, "inside", compute_empty_cells=False)
    assert np.isnan(got[1, 2]) and got[1, 1] == np.float32(6.875) and np.isnan(got).sum() == 15


def test_crop_takes_the_window_clipped_to_the_map():
    got = R.window_expression(A, f"meanOfFinites({X})", X, 3, "crop")
    assert got[0, 0] == 4.0 and got[3, 4] == 17.0 and got[1, 2] == 8.0 and got[1, 1] == np.float32(6.875) and got[2, 2] == np.float32(13.625)
    assert got[0, 2] == 5.0  # 2, 3, 4, 7, 9: the NaN is skipped
    assert not np.isnan(got).any()
    cells = R.window_expression(A, "sum(1)", X, 3, "crop")  # a scalar counts once per cell of W
    assert same(cells, [[4, 6, 6, 6, 4], [6, 9, 9, 9, 6], [6, 9, 9, 9, 6], [4, 6, 6, 6, 4]])
    got = R.window_expression(A, f"meanOfFinites({X})", X, 3, "crop", compute_empty_cells=False)
    assert np.isnan(got[1, 2]) and np.isnan(got).sum() == 1 and got[0, 0] == 4.0
    assert R.window_expression(A, f"sum({X})", X, 3, "crop")[0, 0] == 16.0 and np.isnan(R.window_expression(A, f"sum({X})", X, 3, "crop")[0, 1])


def test_empty_pads_with_nan():
    assert same(R.window_expression(A, "sum(1)", X, 3, "empty"), np.full((4, 5), 9.0))
    assert np.isnan(R.window_expression(A, f"sum({X})", X, 3, "empty")).all()  # the padding or the NaN cell poisons every window
    got = R.window_expression(A, f"numberOfFinites({X})", X, 3, "empty")
    assert same(got, [[4, 5, 5, 5, 4], [6, 8, 8, 8, 6], [6, 8, 8, 8, 6], [4, 6, 6, 6, 4]])
    assert same(R.window_expression(A, f"meanOfFinites({X})", X, 3, "empty"), R.window_expression(A, f"meanOfFinites({X})", X, 3, "crop"))
    assert np.isnan(R.window_expression(A, f"numberOfFinites({X})", X, 3, "empty", compute_empty_cells=False)[1, 2])


def test_mean_pads_with_the_mean_of_the_clipped_window():
    got = R.window_expression(A, f"sum({X})", X, 3, "mean")
    assert got[0, 0] == 36.0   # 1 + 2 + 6 + 7 and five cells of their mean, 4
    assert got[3, 4] == 153.0  # 14 + 15 + 19 + 20 and five cells of 17
    assert np.isnan(got[0, 2])  # the NaN cell is a cell of the map: it is not padded
    got = R.window_expression(A, f"sumOfFinites({X})", X, 3, "mean")
    assert got[0, 2] == 40.0   # 2 + 3 + 4 + 7 + 9 and three cells of their mean, 5
    assert got[1, 1] == 55.0   # a whole window: no padding
    assert same(R.window_expression(A, "sum(1)", X, 3, "mean"), np.full((4, 5), 9.0))
    allnan = np.full((3, 3), NAN, np.float32)
    assert R.window_expression(allnan, f"sumOfFinites({X}) + numberOfFinites({X})", X, 3, "mean")[1, 1] == 0.0
    assert R.window_expression(allnan, f"numberOfFinites({X})", X, 3, "mean")[0, 0] == 0.0  # B has no finite value: the padding is NaN


def test_the_standard_deviation_nests_one_level():
    text = f"sqrt(sumOfFinites(square({X} - meanOfFinites({X}))) ./ numberOfFinites({X}))"
    got = R.window_expression(A, text, X, 3, "crop", compute_empty_cells=False)
    assert got[0, 0] == np.float32(np.sqrt(np.float32(26.0) / np.float32(4.0)))  # 1, 2, 6, 7 around 4: 9 + 4 + 4 + 9
    assert np.isnan(got[1, 2])


@pytest.mark.parametrize("length,res,w", [(0.05, 0.03, 3), (0.1, 0.05, 3), (0.15, 0.05, 3), (0.025, 0.05, 1), (0.02, 0.05, 1), (0.25, 0.05, 5)])
def test_window_length(length, res, w):
    assert R.window_size(window_length=length, resolution=res) == w


def test_window_size_refusals():
    for bad in (0, 2, -1):
        with pytest.raises(ValueError):
            R.window_size(window_size=bad)
    for kw in ({}, {"window_size": 3, "window_length": 0.1}, {"window_length": -0.1}, {"window_length": float("nan")}, {"window_length": float("inf")}):
        with pytest.raises(ValueError):
            R.window_size(resolution=0.05, **kw)
    assert R.window_size(window_size=7) == 7


def test_the_sum_runs_column_by_column():
    """2^60 swallows a 1 in a double.  Column order: (2^60 + 1 + 1) + (1 + 1 + 1) + (-2^60 + 1 + 1) = 0.  Row-major: the big values
    cancel first and the six ones behind them survive: 6."""
    big = np.float32(2.0 ** 60)
    a = np.array([[big, 1, -big], [1, 1, 1], [1, 1, 1]], np.float32)
    assert R.window_expression(a, f"sumOfFinites({X})", X, 3, "inside")[1, 1] == 0.0
    row_major = 0.0
    for v in a.ravel():
        row_major += float(v)
    assert row_major == 6.0
