"""GridMapRosConverter::toOccupancyGrid restated in numpy float32, operation by operation (include/travgpu.h has the
contract).  numpy's float32 `-`, `/` and `*` are IEEE operations rounded once each, which is what the contract asks for."""
import numpy as np


def to_occupancy(layer, data_min, data_max):
    """layer: the rows * cols float32 cells of one map in storage order (element (i, j) at j * rows + i), any shape.
    Returns the int8 data[] of the message: data[n - 1 - k] = cell k."""
    x = np.asarray(layer, dtype=np.float32).reshape(-1)
    mn, mx = np.float32(data_min), np.float32(data_max)
    with np.errstate(all="ignore"):
        rng = np.float32(mx - mn)
        v = ((x - mn) / rng).astype(np.float32)
        nan = np.isnan(v)
        lo = np.where(np.float32(0.0) < v, v, np.float32(0.0)).astype(np.float32)    # std::max(0.0f, v)
        cl = np.where(np.float32(1.0) < lo, np.float32(1.0), lo).astype(np.float32)  # std::min(.., 1.0f)
        val = (np.float32(0.0) + cl * np.float32(100.0)).astype(np.float32)
        cell = np.where(nan, 0, val).astype(np.int64)  # (the conversion truncates; 0 .. 100)
    cell[nan] = -1
    return cell.astype(np.int8)[::-1].copy()


def to_occupancy_reciprocal(layer, data_min, data_max):
    """The same with (v - min) * (1 / (max - min)): what a kernel with a reciprocal instead of the division would give.
    Only the tests' own search for telling cells uses it."""
    x = np.asarray(layer, dtype=np.float32).reshape(-1)
    mn, mx = np.float32(data_min), np.float32(data_max)
    with np.errstate(all="ignore"):
        inv = np.float32(np.float32(1.0) / np.float32(mx - mn))
        v = ((x - mn) * inv).astype(np.float32)
        nan = np.isnan(v)
        lo = np.where(np.float32(0.0) < v, v, np.float32(0.0)).astype(np.float32)
        cl = np.where(np.float32(1.0) < lo, np.float32(1.0), lo).astype(np.float32)
        cell = np.where(nan, 0, (np.float32(0.0) + cl * np.float32(100.0)).astype(np.float32)).astype(np.int64)
    cell[nan] = -1
    return cell.astype(np.int8)[::-1].copy()


def boundary_inputs(data_min, data_max):
    """float32 inputs within a few ulps of the values at which the cell steps from k - 1 to k: where a kernel that multiplies
    by the reciprocal instead of dividing is most likely to give another cell.  (Inputs for a test's own search, not part of the
    restatement.)"""
    mn, mx = np.float32(data_min), np.float32(data_max)
    k = np.arange(1, 101, dtype=np.float64)
    centre = (np.float64(mn) + k / 100.0 * (np.float64(mx) - np.float64(mn))).astype(np.float32)
    out = [centre]
    for direction in (np.float32(-np.inf), np.float32(np.inf)):
        v = centre
        for _ in range(4):
            v = np.nextafter(v, direction)
            out.append(v)
    return np.concatenate(out)


def info_fields(rows, cols, resolution, position):
    """(resolution, width, height, origin[7]) of the message for a map of this geometry."""
    len_x, len_y = rows * float(resolution), cols * float(resolution)
    return (np.float32(resolution), rows, cols,
            (float(position[0]) - 0.5 * len_x, float(position[1]) - 0.5 * len_y, 0.0, 0.0, 0.0, 0.0, 1.0))
