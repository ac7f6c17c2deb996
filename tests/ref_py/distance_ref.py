"""The clearance layer of include/travgpu.h (te_run_distance) as its definition: a brute-force minimum over all pairs of a cell and
a seed, in numpy, written from the contract's text and from nothing under csrc/.

    seeds(layer, mode, threshold)                        -> bool array: which cells are seeds
    cap_cells(max_distance, res)                         -> (cap2, R)
    distance(layer, mode, threshold, max_distance, res)  -> float32 array of the layer's shape

`layer`: one map as a float32 array [rows, cols] (or any 2-D orientation: the definition is symmetric in the axes).
mode: BELOW (seed iff v < float32(threshold)) or ABOVE (v > float32(threshold)), NAN_IS_SEED or-ed in (a NaN cell is a seed
too; without it a NaN cell is never one).  d2 of a cell: the smallest di * di + dj * dj over the seeds, an integer.  cap2: the
largest integer k with float64(k) * (res * res) <= max_distance * max_distance; R = floor(sqrt(cap2)).  A cell with d2 <= cap2
gets float32(sqrt(float64(d2)) * res) -- a seed therefore 0.0 -- and every other cell float32(max_distance)."""
import math

import numpy as np

BELOW, ABOVE, NAN_IS_SEED = 1, 2, 4


def seeds(layer, mode, threshold):
    v = np.asarray(layer, np.float32)
    t = np.float32(threshold)
    with np.errstate(invalid="ignore"):
        s = v < t if (mode & 3) == BELOW else v > t
    if mode & NAN_IS_SEED:
        s = s | np.isnan(v)
    return s


def cap_cells(max_distance, res):
    q, r2 = float(max_distance) * float(max_distance), float(res) * float(res)
    k = int(q / r2)  # a first guess; the rule itself decides
    while float(k + 1) * r2 <= q:
        k += 1
    while k > 0 and float(k) * r2 > q:
        k -= 1
    return k, math.isqrt(k)


def squared_cells(seed):
    """d2 of every cell as int64; a map without a seed: the largest int64 everywhere."""
    seed = np.asarray(seed, bool)
    n0, n1 = seed.shape
    si, sj = np.nonzero(seed)
    out = np.full((n0, n1), np.iinfo(np.int64).max, np.int64)
    if si.size == 0:
        return out
    j = np.arange(n1, dtype=np.int64)
    for i in range(n0):  # all pairs of row i: [n1, seeds]
        d = (np.int64(i) - si.astype(np.int64))[None, :] ** 2 + (j[:, None] - sj.astype(np.int64)[None, :]) ** 2
        out[i] = d.min(axis=1)
    return out


def distance(layer, mode, threshold, max_distance, res):
    return from_squared(squared_cells(seeds(layer, mode, threshold)), max_distance, res)


def from_squared(d2, max_distance, res):
    """The output of d2 = squared_cells(...), which does not depend on the cap."""
    cap2, _ = cap_cells(max_distance, res)
    near = d2 <= cap2
    out = np.full(d2.shape, np.float32(max_distance), np.float32)
    out[near] = (np.sqrt(d2[near].astype(np.float64)) * np.float64(res)).astype(np.float32)
    return out
