"""gridMapFilters/NormalVectorsFilter, `algorithm: raster`, in numpy: the contract of include/travgpu.h (TE_OPT_NORMALS_ALGORITHM)
written from its text, not from the kernel.  grid_map_filters is not in the reference tree: restated, not pinned (DESIGN.md
section 7).

z[i, j] is the input layer (float32) of a rows x cols map, res the resolution (double); x grows towards smaller i, y towards
smaller j.  numpy rounds every double operation on its own (no contraction), and its division and sqrt are correctly rounded:
the order of the operations below IS the contract's."""
import numpy as np


def as_matrix(flat, rows, cols):
    """A layer as the library holds it (flat float32, column-major: element (i, j) at j * rows + i) -> z[i, j]."""
    return np.asarray(flat, np.float32).reshape(cols, rows).T


def as_flat(z):
    return np.ascontiguousarray(np.asarray(z, np.float32).T).reshape(-1)


def _gradient(lo, c, hi, res):
    """One direction: lo / hi the neighbours towards the smaller / larger index.  (gradient, has one)"""
    flo, fhi, fc = np.isfinite(lo), np.isfinite(hi), np.isfinite(c)
    both = flo & fhi
    only_lo = flo & ~fhi & fc
    only_hi = fhi & ~flo & fc
    with np.errstate(all="ignore"):
        g = np.where(both, (hi - lo) / (2.0 * res), np.where(only_lo, (c - lo) / res, (hi - c) / res))
    have = both | only_lo | only_hi
    return np.where(have, g, np.nan), have


def raster_normals(z, res, axis=2):
    """(surface_normal_x, _y, _z) as float32 matrices of z's shape.  axis: normal_vector_positive_axis, 0 x / 1 y / 2 z."""
    z = np.asarray(z, np.float32)
    rows, cols = z.shape
    out = [np.full((rows, cols), np.nan, np.float32) for _ in range(3)]
    if rows < 3 or cols < 3:  # rule 1: the outermost line of cells is never visited
        return tuple(out)
    res = float(res)
    d = z.astype(np.float64)
    c, t, b, l, r = d[1:-1, 1:-1], d[:-2, 1:-1], d[2:, 1:-1], d[1:-1, :-2], d[1:-1, 2:]
    gx, hx = _gradient(t, c, b, res)  # rule 2
    gy, hy = _gradient(l, c, r, res)
    have = hx & hy
    with np.errstate(all="ignore"):
        norm = np.sqrt((gx * gx + gy * gy) + 1.0)  # rule 3
        n = [gx / norm, gy / norm, 1.0 / norm]
        flip = n[axis] < 0.0
        n = [np.where(flip, -v, v) for v in n]
    for k in range(3):
        out[k][1:-1, 1:-1] = np.where(have, n[k], np.nan).astype(np.float32)
    return tuple(out)


def raster_normals_flat(flat, rows, cols, res, axis=2):
    """The same on and to flat column-major layers (one map)."""
    return tuple(as_flat(v) for v in raster_normals(as_matrix(flat, rows, cols), res, axis))
