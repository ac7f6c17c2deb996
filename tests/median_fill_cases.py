"""The shapes, radii and inputs of tests/test_gpu_median_fill.py, kept apart from it so that tests/test_median_plan.py can check --
without a GPU -- that every (rows, cols, r) lands on the kernel its test claims.  No fixture holds -0.0 (the one value whose
sign the contract leaves open)."""
import numpy as np

RES = 0.05
# (rows, cols, batch)
SHAPES = [(5, 7, 1), (70, 37, 1), (130, 33, 1), (40, 21, 3)]
RADII = [0, 1, 3, 7]
# (rows, cols, batch, r, TE_OPT_MEDIAN_ROUTE, the route claimed)
BIG_WINDOW = (96, 80, 1, 40)
STATE_SHAPE = (200, 128, 1)
ROUTE_CLAIMS = [(r_, c_, b_, r, opt, "any" if opt == 2 else "tile") for (r_, c_, b_) in SHAPES for r in RADII for opt in (1, 2)] + \
               [(96, 80, 1, 40, 0, "any"), (96, 80, 1, 1, 2, "any"), (96, 80, 1, 3, 2, "any"), (96, 80, 1, 1, 1, "tile"), (96, 80, 1, 3, 1, "tile"),
                (200, 128, 1, 1, 0, "tile"), (200, 128, 1, 2, 0, "tile")]


def radius_for(r, res=RES):
    """A radius that is r cells at `res`, away from both truncation edges."""
    radius = (r + 0.5) * res
    assert int(radius / res) == r
    return radius


def bag_like(rng, rows, cols):
    """k / 255 like the bag's elevation: smooth, so windows are full of ties."""
    i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    k = np.clip(np.round(60 + 40 * np.sin(i / 9.0) + 30 * np.cos(j / 5.0) + rng.integers(0, 3, (rows, cols))), 0, 255)
    return (np.abs(k) / 255.0).astype(np.float32)  # (abs: np.round leaves a -0.0 where the sum is just below zero)


def values(kind, rng, rows, cols):
    if kind == "bag":
        return bag_like(rng, rows, cols)
    if kind == "mixed_signs":
        return rng.uniform(-3.0, 3.0, (rows, cols)).astype(np.float32)
    if kind == "negatives":
        return (-rng.uniform(0.001, 50.0, (rows, cols))).astype(np.float32)
    if kind == "scales":  # 1e6 beside 1e-6
        return rng.choice(np.array([1e6, 1e-6, -1e6, -1e-6, 1.0, 3e5], np.float32), (rows, cols))
    if kind == "denormals":
        bits = rng.integers(1, 0x007fffff, (rows, cols)).astype(np.uint32) | (rng.integers(0, 2, (rows, cols)).astype(np.uint32) << 31)
        return bits.view(np.float32)
    raise KeyError(kind)


VALUE_KINDS = ["bag", "mixed_signs", "negatives", "scales", "denormals"]


def punch(kind, rng, layer):
    """The hole patterns; returns a copy."""
    a = layer.copy()
    rows, cols = a.shape
    if kind == "none":
        return a
    if kind == "speckle_0.1":
        n = max(1, int(round(0.001 * a.size)))
        a.ravel()[rng.choice(a.size, n, replace=False)] = np.nan
    elif kind == "speckle_5":
        a.ravel()[rng.choice(a.size, max(1, int(round(0.05 * a.size))), replace=False)] = np.nan
    elif kind == "block_30":
        a[: max(1, int(rows * 0.6)), : max(1, int(cols * 0.5))] = np.nan
    elif kind == "all_nan":
        a[:] = np.nan
    elif kind == "single_finite":
        v = a[rows // 2, cols // 3]
        a[:] = np.nan
        a[rows // 2, cols // 3] = v
    elif kind == "frame":  # a finite frame two cells wide around a NaN interior
        a[2:-2, 2:-2] = np.nan
    elif kind == "inf_cells":
        idx = rng.choice(a.size, max(3, a.size // 20), replace=False)
        a.ravel()[idx[0::3]] = np.inf
        a.ravel()[idx[1::3]] = -np.inf
        a.ravel()[idx[2::3]] = np.nan
    else:
        raise KeyError(kind)
    return a


HOLE_KINDS = ["none", "speckle_0.1", "speckle_5", "block_30", "all_nan", "single_finite", "frame", "inf_cells"]
