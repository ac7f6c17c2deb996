"""gridMapFilters/ThresholdFilter and DuplicationFilter in numpy, written from the contract in include/travgpu.h
(te_run_threshold, te_copy_layer): the yardstick of the device filters and of the two fused opcodes of the expression
evaluator.  float32 in, float32 out; the threshold and the replacement are rounded to float32 first, a NaN cell stays NaN
(both comparisons are false for it), and -0.0 compares equal to +0.0."""
import numpy as np


def threshold(values, mode, thr, set_to):
    """mode "lower": v < thr ? set_to : v;  "upper": v > thr ? set_to : v.  Returns a new float32 array."""
    v = np.asarray(values, np.float32)
    t, s = np.float32(thr), np.float32(set_to)
    with np.errstate(invalid="ignore"):
        hit = v < t if mode == "lower" else v > t
    out = v.copy()
    out[hit] = s
    return out


def thresholds(values, steps):
    """The steps [(mode, thr, set_to), ...] one after the other."""
    out = np.asarray(values, np.float32)
    for mode, thr, set_to in steps:
        out = threshold(out, mode, thr, set_to)
    return out


def threshold_region(values, mode, thr, set_to, row0, col0, h, w):
    """On the rectangle of one map stored [col][row]; every other cell keeps its bits."""
    out = np.asarray(values, np.float32).copy()
    out[col0:col0 + w, row0:row0 + h] = threshold(out[col0:col0 + w, row0:row0 + h], mode, thr, set_to)
    return out


def copy(values):
    return np.asarray(values, np.float32).copy()
