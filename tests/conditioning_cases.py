"""Fixtures of the conditioning tests: terrain at an altitude, relief of tens of metres across a strip's window,
resolutions far from 0.05 m, a map origin far from zero, and the two rank-rule inputs with a wide margin.

A plain module (no fixtures of pytest's, no conftest): tests/test_conditioning_ref.py admits every entry on the CPU -- the
oracle alone must lie within TOL / 4 of the exact model (tests/ref_py/normals_ref.py) --, tests/test_gpu_conditioning.py
runs the admitted entries through every kernel route their shape can take.

Shapes.  200 rows give the marching kernels (64 lanes along i) four block columns, the last shifted left to end at the
map's edge: n3_plan_edges (te_n3_plan.h) makes the first and the last edge columns, which run the general tail on every
row, and leaves two INTERIOR columns up to R = 5 and one at R = 9 -- the closed-form tail D = N Szz - Sz^2, the TIES
interior path and the hole queue of the sparse march run only there (tests/test_conditioning_ref.py asks the plan's own
code, tests/cpu/n3_plan_check.cpp, that every marching fixture has an interior column).  The march runs along j.

Strip length.  How long a strip the march slides before it starts again from direct sums is decided per launch by
n3_plan_strips: the smallest height from 8 rows up whose block count fits the device's resident slots divided by the number
of maps, at most 512 rows (the bound of its search loop; the header names no constant for it), and 32 (kN3ShortStripRows)
where unobserved regions were counted.  One map of this size gets strips of 8 rows (4 in the edge columns).  A batch of
LONG_STRIP_MAPS identical copies leaves each map 9 to 12 slots: the strips of the 320-column fixtures (LONG_STRIP) then
are 80 to 319 rows long, whatever of 9 .. 12 x 256 slots the device has -- also asked of the plan's own code --, and on the
planes along j |z - zref| reaches 45 to 160 m inside one strip at res 0.5.  The full 512 rows need a map 512 + 2R cells
long along j and more blocks than slots; the drift of the slid moments per row is the same.
"""
import functools

import numpy as np

ROWS, COLS, MID, LONG = 200, 128, 160, 320
LONG_STRIP_MAPS = 256
FAR = (500.0, -500.0)


def _grid(rows, cols):
    j, i = np.mgrid[0:cols, 0:rows]
    return i.astype(np.float64), j.astype(np.float64)


def _perlin(rows, cols, seed, amplitude, scale=1.0, boxes=6):
    """Perlin terrain with kerbs, heights multiplied by `scale` (terrain that keeps its shape in cells at another res)."""
    from traversability_estimation_amd import synth
    e = synth.with_steps(synth.perlin_elevation(rows, cols, seed=seed, amplitude=amplitude), boxes, seed=seed + 1)
    return e.astype(np.float64) * scale


def _plane(rows, cols, res, gi, gj, seed, noise=2e-3):
    i, j = _grid(rows, cols)
    return res * (gi * i + gj * j) + np.random.default_rng(seed).normal(0.0, noise, (cols, rows))


def _speckle(e, fraction, seed):
    e = e.copy()
    e[np.random.default_rng(seed).random(e.shape) < fraction] = np.nan
    return e


def _radii(res, cells, tie_free=True):
    """Normals and roughness disc of `cells` cells; whole numbers are moved off the circle unless a tie radius is meant."""
    r = cells * res * ((1.0 + 1e-6) if tie_free and float(cells).is_integer() else 1.0)
    return dict(normals_radius=r, rough_radius=r)


def _scaled(res, **radii):
    """Critical values that keep their meaning on terrain scaled from 0.05 m to `res`; step windows of one cell."""
    k = res / 0.05
    return dict(radii, rough_critical=0.05 * k, step_critical=0.12 * k, step_radius1=0.8 * res, step_radius2=0.8 * res)


def _flat(e):
    return np.ascontiguousarray(e, np.float32).reshape(-1)


def cases():
    """Yields (name, rows, cols, res, pos, elev, overrides): elev flat float32 in storage order; overrides are oracle
    parameter fields, plus the key "rank_rule" (popped by the tests) where TE_OPT_NORMALS_RANK_RULE is meant."""
    return iter(_table())


@functools.lru_cache(maxsize=None)
def _table():
    return tuple(_build())


def _build():
    O = (0.0, 0.0)
    # ---- altitude -----------------------------------------------------------------------------------------------------
    yield "alt+64 amp0.05 r9", ROWS, COLS, 0.05, O, _flat(64.0 + _perlin(ROWS, COLS, 11, 0.05)), _radii(0.05, 9)
    yield "alt-64 amp0.6 r5", ROWS, COLS, 0.05, O, _flat(-64.0 + _perlin(ROWS, COLS, 12, 0.6)), _radii(0.05, 5)
    yield "alt+1024 res0.5 r5", ROWS, COLS, 0.5, O, _flat(1024.0 + _perlin(ROWS, COLS, 13, 0.6, 10.0)), _scaled(0.5, **_radii(0.5, 5))
    # (amplitude 1.5: at 0.6 the oracle alone moves one nearly flat cell of this map by 2.7e-6 of slope score, beyond TOL / 4)
    yield "alt+64 origin500 amp1.5 r1.4", ROWS, COLS, 0.05, FAR, _flat(64.0 + _perlin(ROWS, COLS, 14, 1.5)), _radii(0.05, 1.4)
    yield "alt+64 rows48 r14", 48, 256, 0.05, O, _flat(64.0 + _perlin(48, 256, 15, 0.6)), _radii(0.05, 14)
    # ---- relief along the march (j), across the lanes (i), both; rising and falling -----------------------------------
    yield "plane j res0.1 r5", ROWS, LONG, 0.1, O, _flat(_plane(ROWS, LONG, 0.1, 0.0, 1.0, 21)), _radii(0.1, 5)
    yield "plane j res0.5 r9", ROWS, LONG, 0.5, O, _flat(_plane(ROWS, LONG, 0.5, 0.0, 1.0, 22)), _radii(0.5, 9)
    yield "plane j res0.5 alt+64 r5", ROWS, LONG, 0.5, O, _flat(64.0 + _plane(ROWS, LONG, 0.5, 0.0, 1.0, 27)), _radii(0.5, 5)
    s = float(np.sqrt(0.5))
    for res in (0.1, 0.5):
        yield f"plane i res{res:g} r9", ROWS, COLS, res, O, _flat(_plane(ROWS, COLS, res, 1.0, 0.0, 23)), _radii(res, 9)
        yield f"plane diagonal res{res:g} r5", ROWS, COLS, res, O, _flat(_plane(ROWS, COLS, res, s, s, 24)), _radii(res, 5)
    yield "plane j falling res0.5 r5", ROWS, MID, 0.5, O, _flat(_plane(ROWS, MID, 0.5, 0.0, -1.0, 25)), _radii(0.5, 5)
    yield "plane j res0.5 rows48 r14", 48, LONG, 0.5, O, _flat(_plane(48, LONG, 0.5, 0.0, 1.0, 26)), _radii(0.5, 14)
    # ---- relief with holes ----------------------------------------------------------------------------------------------
    e = 64.0 + _plane(ROWS, MID, 0.5, 0.0, 1.0, 31)
    e[0:14, 0:40] = np.nan        # the first lanes of the strips at the top of the map: zref comes from a later lane
    e[60:90, :] = np.nan          # whole rows: strips that start inside find no valid cell in their first rows at all
    e[110:140, 50:150] = np.nan   # the first rows of strips of the interior columns and of the shifted last one
    yield "plane j res0.5 blocks r5", ROWS, MID, 0.5, O, _flat(e), _radii(0.5, 5)
    yield "plane j res0.5 speckle 0.1% r5", ROWS, MID, 0.5, O, _flat(_speckle(_plane(ROWS, MID, 0.5, 0.0, 1.0, 32), 0.001, 33)), _radii(0.5, 5)
    yield "plane j res0.5 speckle 5% r5", ROWS, MID, 0.5, O, _flat(_speckle(_plane(ROWS, MID, 0.5, 0.0, 1.0, 34), 0.05, 35)), _radii(0.5, 5)
    # ---- resolution: 0.005, 0.5 and 2 m, each with 1.4, 5 and 9 cells and a whole-cell radius ---------------------------
    for res, tie in ((0.005, 3), (0.5, 4), (2.0, 4)):
        k = res / 0.05
        terrain = _flat(_perlin(ROWS, COLS, 41, 0.6, k))
        for cells in (1.4, 5, 9):
            yield f"res{res:g} r{cells:g}", ROWS, COLS, res, O, terrain, _scaled(res, **_radii(res, cells))
        yield f"res{res:g} tie{tie:g}", ROWS, COLS, res, O, terrain, _scaled(res, **_radii(res, tie, tie_free=False))
    # ---- map origin on a tie radius ---------------------------------------------------------------------------------------
    yield "alt+64 origin500 tie3", ROWS, COLS, 0.05, FAR, _flat(64.0 + _perlin(ROWS, COLS, 51, 0.6)), _radii(0.05, 3, tie_free=False)
    # ---- rank rule: rank 2 exactly, and rank 3 by a wide gap -----------------------------------------------------------
    # The plane is z = y on a map whose origin puts y at 1024 m and above: every coordinate is dyadic and the z column of every
    # point equals its y column bit for bit, so the centred scatter matrix has two identical rows whatever the disc's mean
    # rounds to -- rank 2 exactly on clipped discs too.  (z = 1024 + 0.25 i + 0.5 j at the origin is NOT such an input: the
    # mean of a disc clipped by the map's border is no dyadic number, the third pivot of the oracle's scatter matrix is
    # rounding noise of about 1e-16 of the first, above its threshold of 3 eps on 711 border cells of a 96 x 256 map's 24 576 and below the
    # device's 1e-12 on all of them -- the band between the two thresholds, which is left alone.)
    pos = (0.0, 1024.0)
    y = pos[1] + (0.5 * COLS * 0.5 - 0.25) - 0.5 * _grid(ROWS, COLS)[1]
    yield "rank rule exact plane r5", ROWS, COLS, 0.5, pos, _flat(y), dict(_radii(0.5, 5), rank_rule=1)
    noisy = y + np.random.default_rng(61).normal(0.0, 0.01, y.shape)
    yield "rank rule noisy plane r5", ROWS, COLS, 0.5, pos, _flat(noisy), dict(_radii(0.5, 5), rank_rule=1)


def names():
    return [c[0] for c in _table()]


def case(name):
    return next(c for c in _table() if c[0] == name)


# the fixtures whose march direction is long enough for the long-strip runs (a batch of LONG_STRIP_MAPS copies)
LONG_STRIP = ("plane j res0.1 r5", "plane j res0.5 r9", "plane j res0.5 alt+64 r5")
