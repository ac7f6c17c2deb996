"""The reach of the region filters (csrc/te_region_plan.h), proved sufficient and tight with the numpy references alone
(tests/ref_py/median_fill_ref.py, tests/ref_py/radius_filter_ref.py), without a GPU: cells inside a rectangle change, the whole-map
reference runs before and after, and outputs and fill mask may differ only inside the rectangle the plan says a region call
writes -- which tests/cpu/region_plan_check.cpp prints.  For one case per filter a cell on the boundary ring of that rectangle
does differ: the reach is not padded."""
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.ref_py import median_fill_ref as M
from tests.ref_py import radius_filter_ref as R
from tests.ref_py.grid_map_ref import GridMapRef

SRC = os.path.join(ROOT, "tests", "cpu", "region_plan_check.cpp")
INC = os.path.join(ROOT, "traversability_estimation_amd", "csrc")
ROWS, COLS, RES = 23, 17, 0.05
# (row0, col0, h, w): a corner, an edge, one interior cell, the whole map
RECTS = [(0, 0, 4, 3), (ROWS - 3, 5, 3, 6), (11, 8, 1, 1), (0, 0, ROWS, COLS)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("region_plan") / "region_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O2", "-I", INC, "-I", os.path.join(ROOT, "include"), SRC, "-o", out], check=True, timeout=300)
    return out


def planned(exe, *args):
    r = subprocess.run([exe] + [repr(a) if isinstance(a, float) else str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    f = r.stdout.split()
    return int(f[1]), tuple(int(v) for v in f[2:6])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def layer(seed, holes=0.25):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, (ROWS, COLS)).astype(np.float32)
    a[rng.random(a.shape) < holes] = np.nan
    a[9:15, 3:8] = np.nan
    a[2, 11], a[17, 4], a[20, 15] = np.inf, -np.inf, np.inf
    return a


def changed(a, rect, seed):
    r0, c0, h, w = rect
    rng = np.random.default_rng(seed)
    b = a.copy()
    t = rng.uniform(-1.0, 1.0, (h, w)).astype(np.float32)
    t[rng.random(t.shape) < 0.4] = np.nan
    b[r0:r0 + h, c0:c0 + w] = t
    return b


def outside(rect):
    m = np.ones((ROWS, COLS), bool)
    m[rect[0]:rect[0] + rect[2], rect[1]:rect[1] + rect[3]] = False
    return m


def ring(rect):
    """the cells of rect that touch its border"""
    m = ~outside(rect)
    inner = np.zeros_like(m)
    inner[rect[0] + 1:rect[0] + rect[2] - 1, rect[1] + 1:rect[1] + rect[3] - 1] = True
    return m & ~inner


_FILL = {}


def fill(a, r_fill, k, fev, r_exist):
    key = (a.tobytes(), r_fill, k, fev, r_exist)
    if key not in _FILL:
        _FILL[key] = M.median_fill(a, RES, (r_fill + 0.5) * RES, fev, (r_exist + 0.5) * RES, k)
    return _FILL[key]


@pytest.mark.parametrize("fev", [False, True])
@pytest.mark.parametrize("r_fill", [0, 1, 2])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_median_fill_changes_stay_inside_the_planned_rectangle(exe, k, r_fill, fev):
    r_exist = 3 if fev else 0  # (beyond r_fill + 2 k for k = 0: the existing radius decides the reach there)
    base = layer(100 + 10 * k + r_fill)
    out0, mask0 = fill(base, r_fill, k, fev, r_exist)
    for n, rect in enumerate(RECTS):
        reach, out_rect = planned(exe, "median", ROWS, COLS, r_fill, r_exist if fev else -1, k, 0, *rect)
        assert reach == max(r_fill + 2 * k, r_exist if fev else 0)
        assert out_rect == (max(rect[0] - reach, 0), max(rect[1] - reach, 0), min(rect[0] + rect[2] + reach, ROWS) - max(rect[0] - reach, 0),
                            min(rect[1] + rect[3] + reach, COLS) - max(rect[1] - reach, 0))
        out1, mask1 = M.median_fill(changed(base, rect, n), RES, (r_fill + 0.5) * RES, fev, (r_exist + 0.5) * RES, k)
        o = outside(out_rect)
        assert np.array_equal(bits(out0)[o], bits(out1)[o]), (rect, out_rect)
        assert np.array_equal(mask0[o], mask1[o]), (rect, out_rect)


@pytest.mark.parametrize("op", [R.MEAN, R.MIN])
@pytest.mark.parametrize("cells", [0.0, 1.5, 2.0, 3.0])
def test_radius_filter_changes_stay_inside_the_planned_rectangle(exe, cells, op):
    gm = GridMapRef(ROWS, COLS, RES, (0.0123, -0.0371))
    base = layer(200 + int(10 * cells))
    out0 = R.radius_filter(base, gm, cells * RES, op)
    for n, rect in enumerate(RECTS):
        reach, out_rect = planned(exe, "radius", op, ROWS, COLS, cells * RES, RES, 0, *rect)
        assert reach == int(cells)
        out1 = R.radius_filter(changed(base, rect, n), gm, cells * RES, op)
        o = outside(out_rect)
        assert np.array_equal(bits(out0)[o], bits(out1)[o]), (rect, out_rect)


def test_the_reach_of_the_fill_is_tight(exe):
    # k = 0: a 5 x 5 block of holes in a finite map; its centre sees no finite cell within 2 and stays a hole until a corner of the
    # block, 2 cells away on both axes, becomes finite
    a = np.ones((ROWS, COLS), np.float32)
    a[8:13, 6:11] = np.nan
    b = a.copy()
    b[12, 10] = 5.0
    reach, out_rect = planned(exe, "median", ROWS, COLS, 2, -1, 0, 0, 12, 10, 1, 1)
    assert reach == 2 and out_rect == (10, 8, 5, 5)
    out0, mask0 = M.median_fill(a, RES, 2.5 * RES, False, 0.0, 0)
    out1, mask1 = M.median_fill(b, RES, 2.5 * RES, False, 0.0, 0)
    assert np.isnan(out0[10, 8]) and out1[10, 8] == 5.0 and not mask0[10, 8] and mask1[10, 8]
    assert ring(out_rect)[10, 8]
    # k = 1, r_fill = 1: one finite cell survives no opening, a 3 x 3 finite block does.  Completing the block at its corner (9, 9)
    # sets the mask 2 k + r_fill = 3 cells away on the far side, at (12, 12) -- and fills that hole
    a = np.full((ROWS, COLS), np.nan, np.float32)
    a[9:12, 9:12] = 2.0
    a[9, 9] = np.nan
    b = a.copy()
    b[9, 9] = 2.0
    reach, out_rect = planned(exe, "median", ROWS, COLS, 1, -1, 1, 0, 9, 9, 1, 1)
    assert reach == 3 and out_rect == (6, 6, 7, 7)
    out0, mask0 = M.median_fill(a, RES, 1.5 * RES, False, 0.0, 1)
    out1, mask1 = M.median_fill(b, RES, 1.5 * RES, False, 0.0, 1)
    assert not mask0.any() and mask1[12, 12] and ring(out_rect)[12, 12]
    assert np.isnan(out0[12, 12]) and out1[12, 12] == 2.0  # the hole 3 cells away on both axes is filled
    assert np.isnan(out0[12, 11]) and out1[12, 11] == 2.0
    assert ring(out_rect)[12, 11]


@pytest.mark.parametrize("op", [R.MEAN, R.MIN])
def test_the_reach_of_the_radius_filters_is_tight(exe, op):
    gm = GridMapRef(ROWS, COLS, RES, (0.0, 0.0))
    a = np.ones((ROWS, COLS), np.float32)
    b = a.copy()
    b[11, 8] = -3.0
    for cells in (1.5, 2.0, 3.0):  # 2.0 and 3.0: the cell on the circle is a tie, decided per centre
        reach, out_rect = planned(exe, "radius", op, ROWS, COLS, cells * RES, RES, 0, 11, 8, 1, 1)
        d = bits(R.radius_filter(a, gm, cells * RES, op)) != bits(R.radius_filter(b, gm, cells * RES, op))
        assert not d[outside(out_rect)].any()
        assert (d & ring(out_rect)).any(), cells
