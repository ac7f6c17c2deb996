"""gridMapFilters/SlidingWindowMathExpressionFilter in numpy: the contract of include/travgpu.h and DESIGN.md section 7, restated
from memory of grid_map_filters and EigenLab (the reference holds neither the filter nor a vector of its).

TEST INFRASTRUCTURE.  The parser is the one of tests/ref_py/expression_ref.py; what differs is the contract's rule 4 (one
variable, a scalar result, one level of nesting) and rule 5 (the reductions).  Vectorised over the cells: a map is an array
[rows, cols, w, w] that holds the w x w window of every cell, a scalar is [rows, cols, 1, 1]; `member` marks the entries that
belong to W (all of them but under `crop`, where W is the window clipped to the map).  A reduction walks the columns of the
window in ascending order, each column's rows in ascending order with a float64 sum that starts at 0.0, and adds the column
sums in column order -- the order the contract defines, so that the device's bits can be asked for.

    window_size(window_size, window_length, resolution) -> w                       (rule 2)
    window_expression(layer, text, name, w, edge, compute_empty_cells) -> float32  (rows, cols)

Layers are numpy arrays indexed [row i, column j].
"""
import math

import numpy as np

from tests.ref_py import expression_ref as E

EDGES = ("inside", "crop", "empty", "mean")


def window_size(window_size=None, window_length=None, resolution=None):
    if (window_size is None) == (window_length is None):
        raise ValueError("exactly one of window_size and window_length")
    if window_length is not None:
        if not (math.isfinite(window_length) and window_length >= 0.0):
            raise ValueError("window_length must be finite and not negative")
        q = window_length / resolution
        w = int(math.floor(q + 0.5))  # std::round of a non-negative double: halves away from zero
        if w % 2 == 0:
            w += 1
    else:
        w = int(window_size)
    if w < 1 or w % 2 == 0:
        raise ValueError("the window size must be odd and at least 1")
    return w


def _fold(values, member, kind):
    """Rule 5 over the last two axes of `values` [rows, cols, wr, wc] (float32) where `member`: -> (sum, count, min, max)."""
    rows, cols, wr, wc = values.shape
    finite = np.isfinite(values)
    takes_all = kind in ("sum", "mean")
    total = np.zeros((rows, cols), np.float64)
    count = np.zeros((rows, cols), np.int64)
    with np.errstate(all="ignore"):
        for c in range(wc):
            col = np.zeros((rows, cols), np.float64)
            for r in range(wr):
                take = member[:, :, r, c] & (finite[:, :, r, c] | takes_all)
                np.add(col, values[:, :, r, c].astype(np.float64), out=col, where=take)
            has_column = member[:, :, :, c].any(axis=2)
            np.add(total, col, out=total, where=has_column)
        ok = member & finite
        count = ok.sum(axis=(2, 3))
        least = np.where(ok, values, np.inf).min(axis=(2, 3))
        most = np.where(ok, values, -np.inf).max(axis=(2, 3))
    return total, count, least, most


def _reduce(kind, values, member):
    total, count, least, most = _fold(values, member, kind)
    cells = member.sum(axis=(2, 3)).astype(np.float64)
    nan = np.float32(np.nan)
    with np.errstate(all="ignore"):
        if kind in ("sum", "sumOfFinites"):
            out = total.astype(np.float32)
        elif kind == "mean":
            out = (total / cells).astype(np.float32)
        elif kind == "meanOfFinites":
            out = np.where(count > 0, (total / np.maximum(count, 1)).astype(np.float32), nan)
        elif kind == "minOfFinites":
            out = np.where(count > 0, least, nan)
        elif kind == "maxOfFinites":
            out = np.where(count > 0, most, nan)
        else:
            out = count.astype(np.float32)
    return np.asarray(out, np.float32)


class _WindowParser(E._Parser):
    def __init__(self, text, name, windows, member):
        super().__init__(text, {name: windows})
        self.name, self.member, self.depth = name, member, 0

    def scalar(self, v):
        return False, np.full(self.shape[:2] + (1, 1), v, dtype=np.float32)

    def primary(self):
        self.ws()
        m = E._NAME.match(self.s, self.i)
        if m and m.group(0) in E.LAYER_NAMES and m.group(0) != self.name:
            raise E.ExprError("BAD_PARAM", f"{m.group(0)} is not the input layer")
        if m and m.group(0) in E._REDUCTIONS:
            kind = m.group(0)
            self.i = m.end()
            if not self.take("("):
                raise E.ExprError("BAD_PARAM", f"'(' expected behind {kind}")
            if self.depth >= 2:
                raise E.ExprError("BAD_PARAM", "reductions nest one level at most")
            self.depth += 1
            a = self.expr()
            self.depth -= 1
            self.close()
            full = np.broadcast_to(a[1], self.shape)  # (a scalar argument counts once per cell of W)
            return False, _reduce(kind, full, self.member)[:, :, None, None]
        return super().primary()


def windows_of(layer, w, edge):
    """-> (W [rows, cols, w, w] float32, member [rows, cols, w, w] bool, whole [rows, cols] bool: the rectangle lies inside the map)."""
    a = np.ascontiguousarray(layer, np.float32)
    rows, cols = a.shape
    m = (w - 1) // 2
    pad = np.pad(a, m, constant_values=np.nan)
    inmap = np.pad(np.ones((rows, cols), bool), m, constant_values=False)
    win = np.lib.stride_tricks.sliding_window_view(pad, (w, w))
    inside = np.lib.stride_tricks.sliding_window_view(inmap, (w, w))
    whole = inside.all(axis=(2, 3))
    if edge in ("inside", "crop"):
        return win, inside, whole
    member = np.ones_like(inside)
    if edge == "mean":
        fill = _reduce("meanOfFinites", win, inside)  # float32 meanOfFinites(B), NaN without a finite value
        win = np.where(inside, win, fill[:, :, None, None]).astype(np.float32)
    return win, member, whole


def window_expression(layer, text, name="elevation", w=3, edge="inside", compute_empty_cells=True):
    """-> float32 (rows, cols).  Raises expression_ref.ExprError as the library refuses (kind BAD_PARAM / UNSUPPORTED)."""
    assert edge in EDGES and w >= 1 and w % 2 == 1
    a = np.ascontiguousarray(layer, np.float32)
    win, member, whole = windows_of(a, w, edge)
    p = _WindowParser(str(text), name, win, member)
    is_map, v = p.top()
    if is_map:
        raise E.ExprError("BAD_PARAM", "the result of a window expression must be a scalar")
    out = np.ascontiguousarray(np.broadcast_to(v, a.shape + (1, 1))[:, :, 0, 0], dtype=np.float32).copy()
    visited = np.ones(a.shape, bool)
    if edge == "inside":
        visited &= whole
    if not compute_empty_cells:
        visited &= np.isfinite(a)
    out[~visited] = np.nan
    return out
