"""The cases of tests/test_gpu_param_routes.py and tests/test_param_routes_ref.py: the parameters no other GPU parity test varies
-- four distinct weights at every place that writes `traversability`, normal_vector_positive_axis x / y on every kind of run, and
fp_max_gap on whole and region runs --, kept apart from the tests so that tests/test_chain_route.py can check, without a GPU,
that every case lands on the route it claims.  Routes are named as tests/cpu/chain_route_check.cpp prints them.

Shapes are those of tests/plugin_filter_cases.py (the smallest at which these kernels can go wrong) and a 130 x 70 map for the
region runs; res 0.05 (0.03 for the second default-YAML route) and a map position that is not the origin.

The weighted sum is written at ten places.  SITES says which weight cases run each of them."""
import collections

import numpy as np

from tests import plugin_filter_cases as K

RES = 0.05
POS = (0.37, -1.21)
PAST_32 = K.PAST_32

# w_scale; w_slope, w_step, w_rough.  All four distinct, and |w_scale| * (|w_slope| + |w_step| + |w_rough|) <= 1: the bound of the
# combined layer (weights_cap, te_ctx_state.h) is then at most the default's (1/3 * 3), so fp_packed_ok (te_fp_route.h) and the
# fixed-point exponent of the footprint pass are the default's and the footprint takes the route it takes under the defaults.
DYADIC = (0.25, 1.5, 0.5, 2.0)     # every product and sum of scores of a few bits is exact
ROUNDING = (0.3, 1.3, 0.6, 1.4)    # every product and sum rounds
SIGNED = (1.0, 1.0, 0.0, -0.5)     # k_combine only: a zero and a negative weight (no bound: not with the footprint).  0 * NaN must stay
#                                    NaN: a chain's step layer is NaN only where the others are, so that is held on uploaded layers
#                                    with independent NaN cells (test_combine_plugin_on_layers_with_independent_nans)
WEIGHT_SETS = {"dyadic": DYADIC, "rounding": ROUNDING, "signed": SIGNED}
DEFAULT_WEIGHTS = (1.0 / 3.0, 1.0, 1.0, 1.0)

# kind: "chain" te_run_chain; "region" te_run_chain, te_upload_tile, te_run_chain_region (route: of the region launch);
#       "filter" te_run_filter normals, slope, roughness (route: of TE_FILTER_NORMALS); "rank" te_run_chain under
#       TE_OPT_NORMALS_RANK_RULE = 1 on the exact-plane map (the shim adds TE_RUN_GENERIC_KERNELS)
# cells: the radii in cells: normals, roughness, step window 1, step window 2
# nan: share of unobserved cells sprinkled over the map; block: an unobserved block that holds whole 64 x 16 tiles
# plateau: a block of constant elevation (slope and roughness scores exactly at their clip 1.0)
# lone: rows 60 and up unobserved but for three pairs of cells more than 33.5 cells from everything else (discs of two points)
# region: (row0, col0, h, w) of the dirty tile; gap: fp_max_gap in metres (None: the default)
# route: (one-kernel chain, step height, step score, normals kernel, fix-up follows, combine)
Case = collections.namedtuple("Case", "name kind rows cols batch res cells axis weights keep generic footprint any_option nan block plateau lone region gap "
                                      "route")


def _case(name, rows, cols, cells, route, kind="chain", batch=1, res=RES, axis=2, weights=DEFAULT_WEIGHTS, keep=False, generic=False, footprint=False,
          any_option=0, nan=0.0, block=False, plateau=False, lone=False, region=None, gap=None):
    cells = tuple(float(v) for v in (cells if len(cells) == 4 else (cells[0], cells[0], cells[1], cells[1])))
    return Case(name, kind, rows, cols, batch, res, cells, axis, weights, keep, generic, footprint, any_option, nan, block, plateau, lone, region, gap, route)


M5 = "march<5>"
LONE_PAIRS = ((5, 100), (45, 100), (25, 128))  # (col, row) of the first cell of each pair of a `lone` map
YAML_005 = (1.0, 0.8)            # robot_filter_parameter.yaml at res 0.05: a one-cell tie radius, single-cell step windows
YAML_003 = (0.05 / 0.03, 0.04 / 0.03)  # ... at res 0.03: a nine-point disc, five-point step windows

# ---- weights ---------------------------------------------------------------------------------------------------------------------
# (template, the sites of DESIGN.md 4.7 it runs -- each shown by a library built with that site's weights exchanged, which fails
# the template's tests).  Site 2 -- the fast tail of k_normals_fixup's list -- runs only behind a kernel that leaves cells to the
# fix-up pass AND combines itself, which is the sliding kernel, on the frame of the map; k_normals on its own (5 x 7, a 17-cell
# radius) has no fix-up pass: every cell is site 1.  With site 2 alone exchanged "5.4 on 63 x 40" fails and "11.3" does not (nor
# with site 1 exchanged: no cell of it leaves the sliding kernel's own statement, site 4).
_WEIGHT_TEMPLATES = [
    (_case("discs 5.4 and 7.3", 70, 37, (5.4, 7.3, 2.5, 2.5), ("none", M5, M5, "k_normals", 0, "in_normals"), nan=0.03), (1,)),
    (_case("same disc, 5 x 7", 5, 7, (3.6, 2.5), ("none", "generic", "generic", "k_normals", 0, "in_normals")), (1,)),
    (_case("17.2", 70, 37, (17.2, 2.5), ("none", M5, M5, "k_normals", 0, "in_normals"), nan=0.03, plateau=True), (1,)),
    (_case("5.4 on 70 x 37", 70, 37, (5.4, 2.5), ("none", M5, M5, "k_normals3-dense", 1, "k_combine"), nan=0.03), (3,)),
    (_case("tie 5", 130, 33, (5.0, 2.5), ("none", M5, M5, "k_normals3-TIES", 1, "k_combine"), nan=0.03), (3,)),
    (_case("5.4 region", 130, 70, (5.4, 2.5), ("none", "generic", "generic", "k_normals_slide", 1, "k_combine"), kind="region", region=(50, 30, 40, 20)), (3,)),
    (_case("5.4 on 63 x 40", 63, 40, (5.4, 2.5), ("none", "generic", "generic", "k_normals_slide", 1, "in_normals"), nan=0.03, plateau=True), (2, 4)),
    (_case("11.3", 70, 37, (11.3, 2.5), ("none", M5, M5, "k_normals_slide<R>", 1, "in_normals"), plateau=True), (4,)),
    # (k_chain_window takes every launch of up to 2^18 cells; k_normals_small writes step and sum only beyond: DESIGN.md's 64 x 4097)
    (_case("default YAML at 0.05 on 64 x 4097", 64, 4097, YAML_005, ("k_normals_small+step+combine", "-", "-", "-", 0, "in_chain"), nan=0.03), (5,)),
    (_case("default YAML at 0.05", 70, 37, YAML_005, ("k_chain_window", "-", "-", "-", 0, "in_chain"), nan=0.03), (6,)),
    (_case("default YAML at 0.03", 70, 37, YAML_003, ("k_chain_window", "-", "-", "-", 0, "in_chain"), res=0.03, nan=0.03), (6,)),
    (_case("past 32", 70, 70, (PAST_32, 2.5), ("none", M5, M5, "any", 0, "in_normals"), any_option=1, nan=0.03, block=True), (8, 9)),
    (_case("past 32 batch", 40, 33, (PAST_32, 2.5), ("none", "generic", "generic", "any", 0, "in_normals"), any_option=1, batch=3), (8, 9)),
    # (k_fa_exact combines only the cells the prefix-moment kernel leaves to it: here the discs of fewer than three points)
    (_case("past 32 lone pairs", 130, 70, (PAST_32, 2.5), ("none", M5, M5, "any", 0, "in_normals"), any_option=1, lone=True), (7, 9)),
    (_case("5.4 footprint", 70, 37, (5.4, 2.5), ("none", M5, M5, "k_normals3-dense", 1, "deferred"), footprint=True, nan=0.03), (10,)),
    (_case("default YAML at 0.05 footprint", 70, 37, YAML_005, ("k_chain_window", "-", "-", "-", 0, "deferred"), footprint=True), (10,)),
    (_case("5.4 on 63 x 40 footprint", 63, 40, (5.4, 2.5), ("none", "generic", "generic", "k_normals_slide", 1, "deferred"), footprint=True, nan=0.03), (10,)),
    (_case("past 32 footprint", 70, 70, (PAST_32, 2.5), ("none", M5, M5, "any", 0, "deferred"), any_option=1, footprint=True, block=True), (10,)),
]


def _weighted(c, set_name):
    return c._replace(name="%s, %s weights" % (c.name, set_name), weights=WEIGHT_SETS[set_name])


WEIGHTS = [_weighted(c, s) for c, _ in _WEIGHT_TEMPLATES for s in ("dyadic", "rounding")]
WEIGHTS.append(_weighted(_WEIGHT_TEMPLATES[3][0], "signed"))
assert WEIGHTS[-1].route[5] == "k_combine"
SITES = {site: [_weighted(c, s).name for c, sites in _WEIGHT_TEMPLATES if site in sites for s in ("dyadic", "rounding")] for site in range(1, 11)}

# the combine kinds and the normals kernels the weight cases have to reach between them (tests/test_chain_route.py)
WEIGHT_COMBINES = {"in_normals", "k_combine", "deferred", "in_chain"}
WEIGHT_KERNELS = {"k_normals", "k_normals3-dense", "k_normals3-TIES", "k_normals_slide", "k_normals_slide<R>", "any",
                  "k_normals_small+step+combine", "k_chain_window"}  # (a one-kernel chain is named by its kernel)

# ---- normal_vector_positive_axis x / y ---------------------------------------------------------------------------------------------
# every run takes k_normals (plan_normals), also where axis z takes a one-kernel chain (the default-YAML radii) or a march
_N = "k_normals"
_AXIS_TEMPLATES = [
    _case("one disc", 70, 37, (5.4, 2.5), ("none", M5, M5, _N, 0, "in_normals"), nan=0.03),
    _case("discs 5.4 and 7.3", 130, 33, (5.4, 7.3, 2.5, 2.5), ("none", M5, M5, _N, 0, "in_normals"), keep=True, nan=0.03),
    _case("tie 5", 70, 37, (5.0, 2.5), ("none", M5, M5, _N, 0, "in_normals"), keep=True),
    _case("batch", 40, 33, (3.6, 2.5), ("none", "generic", "generic", _N, 0, "in_normals"), keep=True, batch=3),
    _case("kept", 64, 40, (5.4, 2.5), ("none", M5, M5, _N, 0, "in_normals"), keep=True, nan=0.03),
    _case("generic flag", 70, 37, (5.4, 2.5), ("none", "generic", "generic", _N, 0, "in_normals"), keep=True, generic=True),
    _case("footprint", 70, 37, (5.4, 2.5), ("none", M5, M5, _N, 0, "deferred"), keep=True, footprint=True, nan=0.03),
    _case("3 x 200", 3, 200, (3.6, 2.5), ("none", "generic", "generic", _N, 0, "in_normals"), keep=True),
    _case("200 x 3", 200, 3, (3.6, 2.5), ("none", M5, M5, _N, 0, "in_normals"), keep=True),
    _case("filter calls", 130, 33, (5.4, 2.5), ("none", "-", "-", _N, 0, "none"), kind="filter", keep=True, nan=0.03),
    # (2.5 cells, not the 2 of that test: with the five-row disc of radius 2 the cells along the plateau's straight edges see one cell
    # beyond it, straight ahead, and their normals are sign-free under x / y -- 0.5 % of the map)
    _case("rank rule", 120, 90, (2.5, 0.8), ("none", "generic", "generic", _N, 0, "in_normals"), kind="rank", res=0.0625, keep=True, generic=True),
    _case("region", 130, 70, (5.4, 2.5), ("none", "generic", "generic", _N, 0, "k_combine"), kind="region", keep=True, region=(50, 30, 40, 20)),
    _case("region in the corner", 130, 70, (5.4, 2.5), ("none", "generic", "generic", _N, 0, "k_combine"), kind="region", keep=True, region=(90, 50, 40, 20)),
    # (the YAML's 0.05 m / 0.04 m at res 0.045, not 0.05: there the one-cell tie radius leaves most discs two or three points, rounding
    # decides which, and the collinear ones -- 1 to 3 % of any map -- have a horizontal normal without a sign under x / y)
    _case("default YAML at 0.045", 70, 37, (0.05 / 0.045, 0.04 / 0.045), ("none", "k_step_small", "k_step_small", _N, 0, "in_normals"), res=0.045, keep=True),
    _case("default YAML at 0.03", 70, 37, YAML_003, ("none", "march<1>", "march<1>", _N, 0, "in_normals"), res=0.03, keep=True, nan=0.03),
]
AXIS = [c._replace(name="%s, axis %s" % (c.name, "xy"[a]), axis=a) for c in _AXIS_TEMPLATES for a in (0, 1)]

# ---- fp_max_gap --------------------------------------------------------------------------------------------------------------------
GAPS = (0.0, 0.05, 0.3, 1.0)  # metres: none, one cell, the default, 20 cells
DEFAULT_GAP_GROWTH = 11       # cells te_run_chain_region grows the dirty rectangle by under the default gap: ceil(0.3 / 0.05) + 5
_GAP_ROUTE = ("none", M5, M5, "k_normals_small-CROSS", 0, "deferred")  # (a one-cell normals radius: one steep cell per island)
GAP = [_case("gap %g" % g, 130, 70, (1.0, 2.5), _GAP_ROUTE, footprint=True, gap=g) for g in GAPS]
GAP_REGION = _case("gap 1 region", 130, 70, (1.0, 2.5), ("none", "generic", "generic", "k_normals_small-CROSS", 0, "k_combine"), kind="region", footprint=True, gap=1.0,
                   region=(50, 30, 30, 16))
GAP.append(GAP_REGION)

ALL = WEIGHTS + AXIS + GAP


def case_id(c):
    return c.name.replace(", ", "-").replace(" ", "_")


def seed_of(c):
    """One map per template: the weight sets and the two axes of a template see the same elevation."""
    key = c.name.split(",")[0] + ("|axis" if c.axis != 2 else "|gap" if c.gap is not None else "|weights")
    return 7000 + sum((k + 1) * ord(ch) for k, ch in enumerate(key)) % 5000


def _ground(c, seed, amplitude=0.12):
    rows, cols = c.rows, c.cols
    e = K.terrain(rows, cols, seed, amplitude)
    rng = np.random.default_rng(seed + 1)
    if c.plateau:
        e[cols // 2:cols // 2 + max(2, cols // 3), rows // 8:rows // 8 + rows // 2] = np.float32(0.25)
    if c.nan:
        e[rng.random(e.shape) < c.nan] = np.nan
    if c.lone:
        e[:, 60:] = np.nan
        for (j, i), dz in zip(LONE_PAIRS, (0.03, 0.045, 0.06)):
            e[j, i], e[j, i + 1] = np.float32(0.2), np.float32(0.2 + dz)
    if c.block:  # whole tiles of 64 x 16 cells without a valid centre, and a wide unobserved area beside a disc of 33 cells
        e[16:40, :] = np.nan
    return e


def rank_rule_map():
    """The map of test_bag_golden_vector_every_cell_with_the_2018_plane_rule (tests/test_gpu_chain.py): rolling ground, an exact
    plane of dyadic slopes and a flat plateau with a step around it, at a dyadic resolution."""
    from traversability_estimation_amd import synth
    r2, c2 = 120, 90
    e = synth.perlin_elevation(r2, c2, seed=31).reshape(c2, r2)
    ii, jj = np.meshgrid(np.arange(r2, dtype=np.float32), np.arange(c2, dtype=np.float32))
    e[:, :40] = (np.float32(0.25) * ii + np.float32(0.125) * jj)[:, :40] * np.float32(1.0 / 32)
    e[20:40, 50:80] = np.float32(0.75)
    return np.ascontiguousarray(e, np.float32)


def gap_map(c):
    """Gentle ground with what checkForStep's ray and checkForSlope's count read fp_max_gap for: ditches and unobserved strips 1 to
    24 cells wide behind kerbs of 0.4 m (a ray of 0, 6 or 20 cells does or does not reach the far side), raised kerbs, a ditch 14
    cells wide that ends at the region case's tile (its far side lies in the tile: the mask changes 15 cells outside it), and
    islands of three observed cells in an unobserved patch (one steep cell each: untraversable only when the gap allows none)."""
    rows, cols = c.rows, c.cols
    rng = np.random.default_rng(4711)
    e = K.terrain(rows, cols, 4711, amplitude=0.01).astype(np.float32)
    for k, width in enumerate((1, 2, 3, 5, 7, 10, 14, 19, 24)):
        j0 = 3 + 7 * k
        e[j0:j0 + 5, 4:4 + width] = np.nan if k % 2 else e[j0:j0 + 5, 4:4 + width] - np.float32(0.4)
    e[48:64, 84:100] += np.float32(0.3)   # kerbs higher than fp_critical_step
    e[16:30, 55:75] -= np.float32(0.4)    # the ditch beside the tile of GAP_REGION (cols 30 .., rows 50 ..)
    e[2:30, 100:128] = np.nan
    for k in range(9):                    # the islands: a corner cell with two neighbours, heights a metre apart
        a, b = 5 + 8 * (k % 3), 103 + 8 * (k // 3)
        e[a, b], e[a + 1, b], e[a, b + 1] = rng.uniform(0.0, 0.1), rng.uniform(0.8, 1.2), rng.uniform(-1.2, -0.8)
    return e


def elevation(c):
    """[batch] maps of shape (cols, rows), float32.  Of a batch of three, map 0 is all NaN, map 1 the case's map and map 2
    another terrain with other holes."""
    seed = seed_of(c)
    if c.kind == "rank":
        return [rank_rule_map()]
    if c.gap is not None:
        return [gap_map(c)]
    own = _ground(c, seed)
    if c.batch == 1:
        return [own]
    assert c.batch == 3
    other = K.punch(K.terrain(c.rows, c.cols, seed + 2, 0.18), seed + 3, "inf+rows")
    return [np.full((c.cols, c.rows), np.nan, np.float32), own, other]


def tile(c, elev):
    """The dirty tile of a region case, shape (w, h): new ground; the gap case raises a box that a ray of 20 cells can meet."""
    r0, c0, h, w = c.region
    rng = np.random.default_rng(seed_of(c) + 5)
    t = elev[c0:c0 + w, r0:r0 + h] + rng.normal(0.0, 0.03, (w, h)).astype(np.float32)
    if c.gap is not None:
        t[0:w - 3, 4:h - 4] += np.float32(0.5)
    else:
        t += (0.1 * np.sin(np.arange(h) / 3.0)[None, :] * np.cos(np.arange(w) / 2.0)[:, None]).astype(np.float32)
    return np.ascontiguousarray(t, np.float32)


def params(oracle, c, **over):
    r = [v * c.res for v in c.cells]
    p = dict(normals_radius=r[0], rough_radius=r[1], step_radius1=r[2], step_radius2=r[3], normals_axis=c.axis,
             w_scale=np.float32(c.weights[0]), w_slope=c.weights[1], w_step=c.weights[2], w_rough=c.weights[3])
    if c.gap is not None:
        p["fp_max_gap"] = c.gap
    p.update(over)
    return oracle.default_params(**p)


def weights_cap(w):
    """te_ctx_state.h: the bound of the combined layer in double, of the float32 weights; -1 when a weight is negative."""
    w = [float(np.float32(v)) for v in w]
    return -1.0 if min(w) < 0 else w[0] * (w[1] + w[2] + w[3])


def route_line(c, maps):
    """The case as tests/cpu/chain_route_check.cpp's `params` mode reads it; the hole counts as the upload takes them (a tile
    upload leaves them unknown)."""
    share, clustered = K.hole_facts(maps)
    if c.kind == "region":
        share, clustered = -1.0, False
    r0, c0, h, w = c.region if c.region else (0, 0, 0, 0)
    return "%s %d %d %d %r %r %r %r %r %d %d %d %d %d %r %d %d %d %d %d %d %d" % (
        case_id(c), c.rows, c.cols, c.batch, c.res, c.cells[0], c.cells[1], c.cells[2], c.cells[3], c.axis, c.keep, c.generic, c.any_option,
        c.footprint, share, clustered, c.region is not None, r0, c0, r0 + h, c0 + w, K.FILTER_NORMALS if c.kind == "filter" else 0)


def disc_points(c, elev, radius):
    """Valid points in the disc of every cell, (cols, rows): grid_map's CircleIterator as tests/ref_py/normals_ref.py restates it."""
    from tests.ref_py.normals_ref import Discs, _shift
    valid = np.isfinite(np.asarray(elev, np.float32).reshape(c.cols, c.rows))
    n = np.zeros(valid.shape, np.int64)
    for di, dj, m in Discs(c.rows, c.cols, c.res, POS, radius, check=False).masks():
        n += m & _shift(valid, di, dj)
    return n


def sign_free(c, elev, want):
    """Cells whose normal has no defined sign under the case's axis: the disc holds three points or more and the oracle's
    component on the axis is within 1e-6 of zero, so rounding noise decides between n and -n (in the reference as in the oracle).
    Not among them: the exact UnitZ (0, 0, 1) that NormalVectorsFilter writes itself -- fewer than three points, a failed
    eigenvalue test, the rank rule --, which is never flipped and is compared strictly.  Flat bool array."""
    n = [np.asarray(want[k], np.float32).reshape(-1) for k in ("surface_normal_x", "surface_normal_y", "surface_normal_z")]
    unit_z = (n[0] == 0) & (n[1] == 0) & (n[2] == 1)
    points = disc_points(c, elev, c.cells[0] * c.res).reshape(-1)
    return (points >= 3) & (np.abs(n[c.axis]) <= 1e-6) & ~unit_z
