"""SlopeFilter and RoughnessFilter as stand-alone plugins, restated in numpy: what each makes of normal layers it did not
compute itself (SlopeFilter.cpp:59-88, RoughnessFilter.cpp:73-132), over the whole map in float64.

Layers are flat float32 in storage order, o = j * rows + i; the 2-D views here have shape (cols, rows).  Cell positions are
GridMap::getPositionFromIndex's, evaluated as the reference does, so that a cell exactly on the circle of a whole-cell radius
is in or out as CircleIterator decides it from the rounded positions.

Nothing here is shared with the oracle (oracle/te_oracle.c) or the library: the sums run offset by offset over the whole map,
column offset outermost, where the oracle gathers each cell's disc row by row."""
import numpy as np


def slope_from_nz(nz, crit):
    """SlopeFilter::update on a surface_normal_z layer: NaN where it is not finite, 1 - acos(nz) / crit below the critical
    angle, else 0 -- also where acos is NaN (|nz| > 1: the comparison is false)."""
    nz = np.asarray(nz, np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        angle = np.arccos(nz.astype(np.float64))
        score = np.where(angle < crit, 1.0 - angle / crit, 0.0)
    return np.where(np.isfinite(nz), score, np.nan).astype(np.float32)


def slope_angle(nz):
    """acos(nz) in float64, NaN where nz is not finite or beyond [-1, 1] (for a test that keeps clear of the threshold)."""
    with np.errstate(invalid="ignore"):
        return np.arccos(np.asarray(nz, np.float32).reshape(-1).astype(np.float64))


def _positions(n, res, centre):
    return (centre + (0.5 * (n * res) - 0.5 * res)) + res * (-np.arange(n, dtype=np.float64))


def _offsets(rows, cols, res, radius, x, y):
    """Yields (target slices, neighbour slices, member) for every offset of the circle's bounding box: member[j, i] says that
    the neighbour of target cell (i, j) lies within the radius."""
    k = int(np.ceil(radius / res)) + 1
    r2 = radius * radius
    for dj in range(-k, k + 1):
        j0, j1 = max(0, -dj), min(cols, cols - dj)
        if j0 >= j1:
            continue
        dy = y[j0 + dj:j1 + dj] - y[j0:j1]
        for di in range(-k, k + 1):
            i0, i1 = max(0, -di), min(rows, rows - di)
            if i0 >= i1:
                continue
            dx = x[i0 + di:i1 + di] - x[i0:i1]
            member = dx[None, :] * dx[None, :] + dy[:, None] * dy[:, None] <= r2
            if member.any():
                yield (slice(j0, j1), slice(i0, i1)), (slice(j0 + dj, j1 + dj), slice(i0 + di, i1 + di)), member


def roughness_value(elev, nx, ny, nz, rows, cols, res, radius, pos=(0.0, 0.0)):
    """(roughness, number of points) of every cell, float64: sqrt(sum of squared distances to the plane through the disc's
    mean with the cell's normal / (n - 1)).  n = 1 gives 0 / 0 or x / 0 (NaN or inf), n = 0 gives 0 (the reference divides by
    the unsigned n - 1); a NaN in any normal component gives NaN."""
    E = np.asarray(elev, np.float32).reshape(cols, rows).astype(np.float64)
    ok = np.isfinite(E)
    Z = np.where(ok, E, 0.0)
    x, y = _positions(rows, res, pos[0]), _positions(cols, res, pos[1])
    X, Y = np.broadcast_to(x[None, :], (cols, rows)), np.broadcast_to(y[:, None], (cols, rows))
    n = np.zeros((cols, rows), np.int64)
    sx, sy, sz = (np.zeros((cols, rows), np.float64) for _ in range(3))
    for t, s, member in _offsets(rows, cols, res, radius, x, y):
        m = member & ok[s]
        n[t] += m
        sx[t] += np.where(m, X[s], 0.0)
        sy[t] += np.where(m, Y[s], 0.0)
        sz[t] += np.where(m, Z[s], 0.0)
    a, b, c = (np.asarray(v, np.float32).reshape(cols, rows).astype(np.float64) for v in (nx, ny, nz))
    with np.errstate(divide="ignore", invalid="ignore"):
        nd = n.astype(np.float64)
        plane = (sx / nd) * a + (sy / nd) * b + (sz / nd) * c
        total = np.zeros((cols, rows), np.float64)
        for t, s, member in _offsets(rows, cols, res, radius, x, y):
            m = member & ok[s]
            dist = a[t] * X[s] + b[t] * Y[s] + c[t] * Z[s] - plane[t]
            total[t] += np.where(m, dist * dist, 0.0)
        rough = np.sqrt(total / (nd - 1.0))
    rough[n == 0] = 0.0
    return rough.reshape(-1), n.reshape(-1)


def roughness_given(elev, nx, ny, nz, rows, cols, res, radius, crit, pos=(0.0, 0.0)):
    """RoughnessFilter::update with the normals of the layers: NaN where surface_normal_x is not finite (the only layer the
    reference tests), 1 - roughness / crit below the critical value, else 0 -- also where the roughness is NaN."""
    rough, _ = roughness_value(elev, nx, ny, nz, rows, cols, res, radius, pos)
    with np.errstate(invalid="ignore"):
        score = np.where(rough < crit, 1.0 - rough / crit, 0.0)
    return np.where(np.isfinite(np.asarray(nx, np.float32).reshape(-1)), score, np.nan).astype(np.float32)
