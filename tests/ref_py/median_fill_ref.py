"""gridMapFilters/MedianFillFilter in plain numpy: the contract of include/travgpu.h (te_run_median_fill), written from the
contract and not from the kernels.  grid_map_filters is not in the reference tree, so this restatement IS the yardstick; nothing
in it is pinned by a vector the reference holds.

Arrays are (rows, cols): element [i, j] is row i, column j.  (The device layers are column-major, i.e. the transposed array in
C order; the window is a square and the rule symmetric, so the tests transpose once at the border.)

    radius_cells(radius, res)      int(radius / res): the double division, truncated
    opened_mask(valid, k)          k erosions, then k dilations with a 3 x 3 square; cells outside the map do not vote
    fill_mask(layer, r, k)         shouldFill: some cell of the opened mask lies in the cell's clamped window of radius r
    median_fill(layer, ...)        (output layer, fill mask)
"""
import numpy as np


def radius_cells(radius, resolution):
    return int(radius / resolution)


def _window(i, j, r, shape):
    return slice(max(i - r, 0), min(i + r, shape[0] - 1) + 1), slice(max(j - r, 0), min(j + r, shape[1] - 1) + 1)


def window_median(layer, i, j, r):
    """The upper median of the finite values in the clamped window; NaN if there is none."""
    w = layer[_window(i, j, r, layer.shape)].ravel()
    finite = w[np.isfinite(w)]
    n = finite.size
    if n == 0:
        return np.float32(np.nan)
    return np.sort(finite)[n // 2]


def _morph(mask, erode):
    out = np.zeros_like(mask)
    for i in range(mask.shape[0]):
        for j in range(mask.shape[1]):
            w = mask[_window(i, j, 1, mask.shape)]
            out[i, j] = w.all() if erode else w.any()
    return out


def opened_mask(valid, iterations):
    m = np.asarray(valid, bool)
    for _ in range(iterations):
        m = _morph(m, True)
    for _ in range(iterations):
        m = _morph(m, False)
    return m


def fill_mask(layer, r_fill, iterations):
    cleaned = opened_mask(np.isfinite(layer), iterations)
    out = np.zeros(layer.shape, bool)
    for i in range(layer.shape[0]):
        for j in range(layer.shape[1]):
            out[i, j] = cleaned[_window(i, j, r_fill, layer.shape)].any()
    return out


def median_fill(layer, resolution, fill_hole_radius=0.05, filter_existing_values=False, existing_value_radius=0.0,
                num_erode_dilation_iterations=4):
    """(output, fill mask) of one float32 (rows, cols) layer.  Only the input is read; cells that keep their value keep its bits."""
    layer = np.asarray(layer, np.float32)
    r_fill = radius_cells(fill_hole_radius, resolution)
    r_exist = radius_cells(existing_value_radius, resolution)
    mask = fill_mask(layer, r_fill, num_erode_dilation_iterations)
    out = layer.copy()
    finite = np.isfinite(layer)
    for i in range(layer.shape[0]):
        for j in range(layer.shape[1]):
            if not mask[i, j]:
                continue
            if not finite[i, j]:
                out[i, j] = window_median(layer, i, j, r_fill)
            elif filter_existing_values:
                out[i, j] = window_median(layer, i, j, r_exist)
    return out, mask
