"""tests/ref_py/median_fill_ref.py, the numpy restatement the GPU tests compare with, on 5 x 5 cases a reader can check by eye.
Resolution 1.0, so a radius is its number of cells."""
import numpy as np

from tests.ref_py import median_fill_ref as R

N = np.nan


def arr(rows):
    return np.array(rows, np.float32)


def same(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def test_even_count_takes_the_upper_median():
    a = np.full((5, 5), N, np.float32)
    a[2, 1], a[2, 3] = 1.0, 2.0  # the window of (2, 2) at r = 1 holds exactly these two
    out, mask = R.median_fill(a, 1.0, fill_hole_radius=1.0, num_erode_dilation_iterations=0)
    assert out[2, 2] == 2.0
    # (1, 2) sees both as well; (1, 0) sees only the 1.0; (0, 4) sees nothing and stays NaN outside the mask
    assert out[1, 2] == 2.0 and out[1, 0] == 1.0 and np.isnan(out[0, 4]) and not mask[0, 4]
    assert out[2, 1] == 1.0 and out[2, 3] == 2.0
    assert mask.sum() == 15  # rows 1 .. 3, every column: each of them sees (2, 1) or (2, 3)
    assert R.window_median(arr([[4, 1], [3, 2]]), 0, 0, 1) == 3.0  # n = 4: index 2 of 1 2 3 4


def test_window_is_clamped_at_a_corner():
    a = arr([[N, 5, 9, 9, 9],
             [7, 1, 9, 9, 9],
             [9, 9, 9, 9, 9],
             [9, 9, 9, 9, 9],
             [9, 9, 9, 9, N]])
    out, _ = R.median_fill(a, 1.0, fill_hole_radius=1.0, num_erode_dilation_iterations=0)
    assert out[0, 0] == 5.0  # the clamped window holds 5, 7, 1: sorted 1 5 7, index 1
    assert out[4, 4] == 9.0
    expect = a.copy()
    expect[0, 0], expect[4, 4] = 5.0, 9.0
    assert same(out, expect)


def test_square_window_not_a_disc():
    a = np.full((5, 5), N, np.float32)
    a[0, 0] = 3.0
    out, mask = R.median_fill(a, 1.0, fill_hole_radius=2.0, num_erode_dilation_iterations=0)
    assert out[2, 2] == 3.0 and mask[2, 2]  # the corner of the square, 2.83 cells away
    assert mask[:3, :3].all() and mask.sum() == 9


def test_opening_removes_an_isolated_cell_from_the_mask_but_not_from_the_medians():
    a = np.full((5, 5), N, np.float32)
    a[0:3, 0:3] = 1.0   # a 3 x 3 block in the corner survives one opening iteration
    a[4, 4] = 8.0       # an isolated finite cell does not
    a[2, 3] = N
    cleaned = R.opened_mask(np.isfinite(a), 1)
    assert cleaned[0:3, 0:3].all() and cleaned.sum() == 9 and not cleaned[4, 4]
    out, mask = R.median_fill(a, 1.0, fill_hole_radius=1.0, num_erode_dilation_iterations=1)
    # (3, 3) is filled because of the block's corner (2, 2); its median counts the isolated 8.0: finite values 1.0 and 8.0, n = 2
    assert mask[3, 3] and out[3, 3] == 8.0
    # (3, 4) sees only the isolated cell, which is not in the cleaned mask: not filled
    assert not mask[3, 4] and np.isnan(out[3, 4])
    assert not mask[4, 4] and out[4, 4] == 8.0
    # without the opening the isolated cell fills its neighbours
    out0, mask0 = R.median_fill(a, 1.0, fill_hole_radius=1.0, num_erode_dilation_iterations=0)
    assert mask0[3, 4] and out0[3, 4] == 8.0


def test_filter_existing_values():
    a = arr([[1, 1, 1, 1, 1],
             [1, 9, 1, 1, 1],
             [1, 1, 1, N, 1],
             [1, 1, 1, 1, 1],
             [1, 1, 1, 1, 5]])
    keep, _ = R.median_fill(a, 1.0, fill_hole_radius=1.0, filter_existing_values=False, existing_value_radius=1.0, num_erode_dilation_iterations=0)
    assert keep[1, 1] == 9.0 and keep[2, 3] == 1.0
    ident, _ = R.median_fill(a, 1.0, fill_hole_radius=1.0, filter_existing_values=True, existing_value_radius=0.0, num_erode_dilation_iterations=0)
    assert same(ident, keep)  # radius 0: the identity on finite cells
    filt, _ = R.median_fill(a, 1.0, fill_hole_radius=1.0, filter_existing_values=True, existing_value_radius=1.0, num_erode_dilation_iterations=0)
    assert filt[1, 1] == 1.0 and filt[4, 4] == 1.0 and filt[2, 3] == 1.0  # the outliers go; (4, 4): 1 1 1 5, index 2
    assert (filt == 1.0).all()


def test_inf_is_left_out_like_nan_and_untouched_cells_keep_their_bits():
    a = np.full((5, 5), N, np.float32)
    a[2, 2] = np.inf
    a[2, 1] = 4.0
    a[0, 4] = np.frombuffer(np.uint32(0x7fc12345).tobytes(), np.float32)[0]  # a NaN with a payload, outside every window
    out, mask = R.median_fill(a, 1.0, fill_hole_radius=1.0, num_erode_dilation_iterations=0)
    assert out[2, 2] == 4.0  # not finite, and its window holds a finite value
    assert out.view(np.uint32)[0, 4] == 0x7fc12345 and not mask[0, 4]
    b = np.full((5, 5), N, np.float32)
    b[2, 2] = -np.inf
    out, mask = R.median_fill(b, 1.0, fill_hole_radius=1.0, num_erode_dilation_iterations=0)
    assert not mask.any() and same(out, b)  # no finite value anywhere: nothing is filled, -inf stays
