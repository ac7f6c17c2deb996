"""Shared by the GPU tests of the user layers, the layer expressions and the point-wise filters: the two map shapes, the input
with its holes, and the comparisons (bits plus NaN pattern)."""
import numpy as np

RES = 0.05
SHAPES = [(37, 29, 2), (96, 70, 1)]  # rows, cols, batch
WEIGHTED = "(1.0 * traversability_slope + 1.0 * traversability_step + 1.0 * traversability_roughness) / 3.0"


def holed(rows, cols, batch, seed, lo=-1.0, hi=3.0):
    """[batch][cols][rows] float32 with 5 % NaN: scattered cells, a NaN strip along two borders and a NaN block."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(lo, hi, (batch, cols, rows)).astype(np.float32)
    a[rng.random(a.shape) < 0.03] = np.nan
    a[:, :, 0] = np.nan           # the first row of every column
    a[:, cols - 1, : rows // 2] = np.nan
    a[:, cols // 3:cols // 3 + 4, rows // 2:rows // 2 + 5] = np.nan
    return a


def same(a, b):
    """bits plus NaN pattern: every NaN counts as the same value"""
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    an, bn = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(an, bn) and np.array_equal(a[~an].view(np.uint32), b[~bn].view(np.uint32))


def context(capi, rows, cols, batch, pos=(0.0, 0.0)):
    ctx = capi.Context(0)
    ctx.set_params(capi.default_params())
    ctx.set_geometry(rows, cols, batch, RES, pos)
    return ctx


def grid(ctx, layer):
    """the layer as [batch][cols][rows]"""
    return ctx.download(layer).reshape(ctx.batch, ctx.cols, ctx.rows)


# rectangles (row0, col0, h, w) touching each border, and one interior at an odd origin
def rects(rows, cols):
    return [(0, 5, 3, 7), (rows - 6, 2, 6, 5), (4, 0, 9, 2), (7, cols - 3, 5, 3), (11, 9, 13, 6), (0, 0, rows, cols)]
