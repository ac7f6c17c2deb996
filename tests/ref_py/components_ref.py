"""The connected regions of include/travgpu.h (te_run_components / te_run_reachable) as their definition: a brute-force flood fill
in plain Python, written from the contract's text and from nothing under csrc/.

    free(layer, mode, threshold)             -> bool array: which cells are free
    labels(free, connectivity)               -> int64 array: the label of every free cell, -1 on a blocked one
    sizes(layer, mode, threshold, conn)      -> float32 array: te_run_components
    reachable(layer, mode, threshold, conn, starts) -> float32 array: te_run_reachable
    stats(layer, mode, threshold, conn, starts=None) -> (components, free cells, largest component, cells written 1.0)

`layer`: one map as a float32 array [rows, cols].  mode: BELOW (blocked iff v < float32(threshold)) or ABOVE (v > float32(threshold)),
NAN_IS_SEED or-ed in (a NaN cell is blocked too; without it a NaN cell is free); v == threshold is free in both modes.
Neighbours: connectivity 4: (i +- 1, j), (i, j +- 1); 8: the four diagonals as well, whatever lies beside them.  No wrap.  The
fill scans in storage order (column-major: col * rows + row), so a label is the smallest such index of its component."""
import numpy as np

BELOW, ABOVE, NAN_IS_SEED = 1, 2, 4

STEPS = {4: ((-1, 0), (1, 0), (0, -1), (0, 1)),
         8: ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))}


def free(layer, mode, threshold):
    v = np.asarray(layer, np.float32)
    t = np.float32(threshold)
    with np.errstate(invalid="ignore"):
        blocked = v < t if (mode & 3) == BELOW else v > t
    if mode & NAN_IS_SEED:
        blocked = blocked | np.isnan(v)
    return ~blocked


def labels(free_cells, connectivity):
    f = np.asarray(free_cells, bool)
    rows, cols = f.shape
    steps = STEPS[connectivity]
    ok = f.tolist()
    lab = [[-1] * cols for _ in range(rows)]
    for j in range(cols):
        for i in range(rows):
            if not ok[i][j] or lab[i][j] >= 0:
                continue
            mine = j * rows + i
            lab[i][j] = mine
            stack = [(i, j)]
            while stack:
                a, b = stack.pop()
                for da, db in steps:
                    p, q = a + da, b + db
                    if 0 <= p < rows and 0 <= q < cols and ok[p][q] and lab[p][q] < 0:
                        lab[p][q] = mine
                        stack.append((p, q))
    return np.array(lab, np.int64).reshape(rows, cols)


def sizes_of(lab):
    """float32 array: the size of every free cell's component as uint32 -> float32, 0.0 on a blocked cell."""
    out = np.zeros(lab.shape, np.float32)
    ids, inverse, counts = np.unique(lab, return_inverse=True, return_counts=True)
    per_cell = counts[inverse].reshape(lab.shape)
    out[lab >= 0] = per_cell[lab >= 0].astype(np.uint32).astype(np.float32)
    return out


def sizes(layer, mode, threshold, connectivity):
    return sizes_of(labels(free(layer, mode, threshold), connectivity))


def reachable_of(lab, starts):
    rows, cols = lab.shape
    hit = {int(lab[r, c]) for r, c in starts if lab[r, c] >= 0}
    out = np.zeros(lab.shape, np.float32)
    if hit:
        out[np.isin(lab, sorted(hit))] = 1.0
    return out


def reachable(layer, mode, threshold, connectivity, starts):
    return reachable_of(labels(free(layer, mode, threshold), connectivity), starts)


def stats_of(lab, starts=None):
    live = lab[lab >= 0]
    if live.size == 0:
        return (0, 0, 0, 0)
    _, counts = np.unique(live, return_counts=True)
    ones = int(reachable_of(lab, starts).sum()) if starts is not None else 0
    return (int(counts.size), int(live.size), int(counts.max()), ones)


def stats(layer, mode, threshold, connectivity, starts=None):
    return stats_of(labels(free(layer, mode, threshold), connectivity), starts)
