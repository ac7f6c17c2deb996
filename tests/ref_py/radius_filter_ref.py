"""gridMapFilters/MeanInRadiusFilter and MinInRadiusFilter in numpy: the contract of include/travgpu.h and DESIGN.md section 7,
restated from memory of grid_map_filters (the reference holds neither the filters nor a vector of theirs).

TEST INFRASTRUCTURE.  Vectorised over the centres: for each offset (di, dj) -- di ascending outer, dj ascending inner, the order
CircleIterator visits the cells of one window in -- the layer shifted by the offset takes part where the shifted cell is a
cell of the map, lies inside that centre's circle by GridMapRef's own formula (positions and squared distance in double, per
centre), and is finite.  tests/test_radius_filter_ref.py checks it against a literal loop over GridMapRef.circle.

Layers are numpy arrays indexed [row i, column j].
"""
import math

import numpy as np

MEAN, MIN = 1, 2


def _positions(gm, n, k):
    """getPositionFromIndex along axis k for indices 0 .. n - 1, as GridMapRef.position computes it."""
    idx = np.arange(n, dtype=np.float64)
    return gm.pos[k] + (0.5 * gm.length[k] - 0.5 * gm.res) + gm.res * (-idx)


def radius_filter(layer, gm, radius, op):
    """-> float32 (rows, cols).  gm: GridMapRef of the layer's shape."""
    a = np.ascontiguousarray(layer, np.float32)
    rows, cols = a.shape
    assert (rows, cols) == gm.size
    r2 = radius * radius
    x, y = _positions(gm, rows, 0), _positions(gm, cols, 1)
    reach = int(min(math.ceil(radius / gm.res) + 1, max(rows, cols)))
    total = np.zeros((rows, cols), np.float64)
    count = np.zeros((rows, cols), np.int64)
    least = np.full((rows, cols), np.nan, np.float32)
    for di in range(-min(reach, rows - 1), min(reach, rows - 1) + 1):
        ia, ib = max(0, -di), min(rows, rows - di)  # centres whose cell i + di is a row of the map
        dx = x[ia + di:ib + di] - x[ia:ib]
        for dj in range(-min(reach, cols - 1), min(reach, cols - 1) + 1):
            ja, jb = max(0, -dj), min(cols, cols - dj)
            dy = y[ja + dj:jb + dj] - y[ja:jb]
            inside = (dx * dx)[:, None] + (dy * dy)[None, :] <= r2
            if not inside.any():
                continue
            v = a[ia + di:ib + di, ja + dj:jb + dj]
            take = inside & np.isfinite(v)
            if op == MEAN:
                np.add(total[ia:ib, ja:jb], v.astype(np.float64), out=total[ia:ib, ja:jb], where=take)
                count[ia:ib, ja:jb] += take
            else:
                cur = least[ia:ib, ja:jb]
                with np.errstate(invalid="ignore"):
                    lower = take & (np.isnan(cur) | (v < cur) | ((v == cur) & np.signbit(v)))  # -0.0 sorts below +0.0
                cur[lower] = v[lower]
    if op == MIN:
        return least
    out = np.full((rows, cols), np.nan, np.float32)
    some = count > 0
    out[some] = (total[some] / count[some].astype(np.float64)).astype(np.float32)
    return out


def radius_filter_loop(layer, gm, radius, op):
    """The contract literally: one CircleIterator walk per centre."""
    a = np.ascontiguousarray(layer, np.float32)
    rows, cols = a.shape
    out = np.full((rows, cols), np.nan, np.float32)
    for i in range(rows):
        for j in range(cols):
            total, n, least = 0.0, 0, None
            for q in gm.circle(gm.position((i, j)), radius):
                v = a[q]
                if not np.isfinite(v):
                    continue
                total += float(v)
                n += 1
                if least is None or v < least or (v == least and np.signbit(v)):
                    least = v
            if n:
                out[i, j] = np.float32(total / n) if op == MEAN else least
    return out
