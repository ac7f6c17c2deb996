"""The shapes, windows, expressions and inputs of tests/test_gpu_window_expression.py, kept apart from it so that
tests/test_window_plan.py can check -- without a GPU -- that every case lands on the route its GPU test claims.  Hole patterns and
value kinds: tests/median_fill_cases.py."""
import numpy as np

from tests import median_fill_cases as M

RES = M.RES
EDGES = ("inside", "crop", "empty", "mean")
# 5 x 7: smaller than a 9-window; 70 x 37 and 130 x 33: workgroup edges and partial workgroups both ways (32 x 8 cells per
# workgroup); a batch of 3, every map with another hole pattern
SHAPES = [(5, 7, 1), (70, 37, 1), (130, 33, 1), (40, 21, 3)]
BATCH_HOLES = ["all_nan", "inf_cells", "speckle_5"]
WINDOWS = [1, 3, 5, 9]
OFF_LDS_SHAPES = [(5, 7, 1), (70, 37, 1)]  # where the smallest window off the LDS tile is run (read from the plan)

X = "elevation"
STD_DEV = f"sqrt(sumOfFinites(square({X} - meanOfFinites({X}))) ./ numberOfFinites({X}))"
# (text, reductions, outer reductions): compared on the bit patterns
EXACT = [(STD_DEV, 3, 1),
         (f"meanOfFinites({X})", 1, 0),
         (f"maxOfFinites({X}) - minOfFinites({X})", 2, 0),
         (f"sum({X})", 1, 0),
         (f"mean({X})", 1, 0),
         (f"numberOfFinites({X})", 1, 0),
         ("0.25 + 2 * 3", 0, 0),
         (f"2 * meanOfFinites({X}) - minOfFinites({X})", 2, 0)]
EXP_MEAN = f"meanOfFinites(exp({X}))"


def claim(reductions, outer, w, option):
    """The route of a call: what te_window_plan.h decides, restated."""
    if option == 2 or reductions == 0 or outer > 0:
        return "direct"
    if option == 0 and w < 5:
        return "direct"
    return "separable"


def maps(rows, cols, batch, seed, kinds=None, kind="bag"):
    """[batch] maps of value kind `kind`, map n with the hole pattern kinds[n % len(kinds)]."""
    rng = np.random.default_rng(seed)
    kinds = kinds or (BATCH_HOLES if batch > 1 else ["speckle_5"])
    return [M.punch(kinds[n % len(kinds)], rng, M.values(kind, rng, rows, cols)) for n in range(batch)]
