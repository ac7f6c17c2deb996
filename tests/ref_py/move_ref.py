"""te_move_map's contract in numpy, written from the statement in include/travgpu.h, not from te_move_plan.h: the index shift
of GridMap::move, the position held afterwards, the moved layer and the rectangles the caller refreshes.

Layers are arrays of shape (cols, rows) -- [col][row], the device's column-major order -- so a shift of (shift_rows, shift_cols)
cells moves old cell [j, i] to [j + shift_cols, i + shift_rows]."""
import math

import numpy as np


def axis_shift(held, requested, res):
    """(int)(s + 0.5 * sign(s)) with s = (requested - held) / res: halves round away from zero."""
    s = (float(requested) - float(held)) / float(res)
    return int(math.trunc(s + 0.5 * ((s > 0) - (s < 0))))


def shift_and_position(res, pos, new_pos):
    kr, kc = axis_shift(pos[0], new_pos[0], res), axis_shift(pos[1], new_pos[1], res)
    if kr == 0 and kc == 0:
        return (0, 0), (pos[0], pos[1])  # upstream returns early: the position stays bit for bit
    return (kr, kc), (pos[0] + kr * res, pos[1] + kc * res)


def moved(layer, shift, fill=np.nan):
    """The layer after the move: `fill` where the source lies outside the old window."""
    a = np.asarray(layer)
    cols, rows = a.shape[-2:]
    kr, kc = shift
    out = np.full(a.shape, fill, a.dtype)
    if abs(kr) < rows and abs(kc) < cols:
        out[..., max(kc, 0):cols + min(kc, 0), max(kr, 0):rows + min(kr, 0)] = a[..., max(-kc, 0):cols + min(-kc, 0), max(-kr, 0):rows + min(-kr, 0)]
    return out


def exposed_mask(rows, cols, shift):
    """(cols, rows) bool: the cells whose source lies outside the old window."""
    return moved(np.zeros((cols, rows), np.uint8), shift, fill=1).astype(bool)


def rectangles(rows, cols, shift):
    """[((row0, col0, h, w), exposed)]: the band of exposed rows over the full width, the band of exposed columns over the rows
    that are left, then on each axis that moved the one-cell line along the opposite border; the whole map when a shift
    reaches the map's extent; nothing for a zero shift."""
    kr, kc = shift
    if kr == 0 and kc == 0:
        return []
    if abs(kr) >= rows or abs(kc) >= cols:
        return [((0, 0, rows, cols), True)]
    out = []
    i_lo, i_hi = max(kr, 0), rows + min(kr, 0)
    if kr:
        out.append(((0 if kr > 0 else i_hi, 0, abs(kr), cols), True))
    if kc:
        out.append(((i_lo, 0 if kc > 0 else cols + kc, i_hi - i_lo, abs(kc)), True))
    if kr:
        out.append(((rows - 1 if kr > 0 else 0, 0, 1, cols), False))
    if kc:
        out.append(((0, cols - 1 if kc > 0 else 0, rows, 1), False))
    return out


def all_exposed(rows, cols, shift):
    return abs(shift[0]) >= rows or abs(shift[1]) >= cols
