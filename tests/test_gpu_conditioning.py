"""Parity under hard conditioning: the fixtures of tests/conditioning_cases.py (terrain at +-64 m and +1024 m, planes of
gradient 1 whose heights span 30 to 160 m, unobserved blocks and speckle on them, res from 0.005 to 2 m, a map origin at
(500, -500), the two rank-rule inputs) through every normals route of DESIGN.md section 4.7 their shape can take, against
the oracle at the project's 1e-5 and against each other.

tests/test_conditioning_ref.py admits the fixtures on the CPU: on each of them the oracle alone stays within TOL / 4 of the
exact model, so a deviation beyond TOL here is the kernel's.

Routes are steered with what the library offers, nothing test-only: the fixture's shape and radius, TE_RUN_KEEP_NORMALS (the
kernel that keeps the normals exists with the dense march only; the slim ring, the sparse march and k_chain_window need a
run without it), a 48-row copy of the map (k_normals_slide), TE_RUN_GENERIC_KERNELS, TE_OPT_FILTER_ANY_RADIUS = 2, a
batch of two maps and a region run over an odd-origin rectangle.  The kernel in a test id is the one plan_chain_route
(te_chain_route.h) gives that input: tests/test_chain_route.py asks the library's own header for every (fixture, route) here
and compares.  What the strip plan gives these shapes -- interior block columns, strip heights --
is asked of the kernels' own header in tests/test_conditioning_ref.py.

Strip length: one map of this size gets strips of 8 rows; test_long_strips runs a batch of LONG_STRIP_MAPS copies of the
320-column planes, which the plan gives strips of 80 to 319 rows (tests/conditioning_cases.py)."""
import os

import numpy as np
import pytest

from tests import conditioning_cases as cc
from tests.helpers import OUT_LAYERS, TOL, assert_layers_match, orient_horizontal_normals, to_te_params
from tests.test_gpu_random import _forgive_rounding_ties_of_the_normal_layer

pytestmark = pytest.mark.gpu

NRM = ("surface_normal_x", "surface_normal_y", "surface_normal_z")
NORMALS_TOL = 1e-5  # like the scores (float32 rounding of a component is 6e-8)


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no MI355X visible"
    return capi


@pytest.fixture(scope="module")
def threads(oracle):
    oracle.set_threads(min(os.cpu_count() or 1, 16))
    yield
    oracle.set_threads(1)


def _split(over):
    over = dict(over)
    return over, bool(over.pop("rank_rule", 0))


def _holes(elev):
    bad = ~np.isfinite(elev)
    return 0.0 if not bad.any() else float(bad.mean())


def _cells(over, res):
    return over["normals_radius"] / res


def kernel_of(name, route):
    """The kernel DESIGN.md section 4.7 names for this fixture on this route (for the test id)."""
    _, rows, cols, res, pos, elev, over = cc.case(name)
    over, rank = _split(over)
    if route == "generic" or rank:
        return "k_normals+k_normals_fixup"
    if route == "any":
        return "k_fa_normals+k_fa_exact"
    c = _cells(over, res)
    tie = abs(c - round(c)) < 1e-9
    if c < 3 and (not tie or c <= 2):  # a whole-map launch of these sizes is one kernel, kept or not, 48 rows or 200
        return "k_chain_window"        # (the region run of batch+region: k_normals_small)
    if route == "rows48" or rows < 64 or c >= 11:
        if tie:  # the TIES march needs 64 rows and nothing else takes a tie radius of three cells and more
            return "k_normals"  # (alone: no fix-up pass behind the generic kernel)
        return "k_normals_slide<R>" if c >= 11 else "k_normals_slide"
    if tie:
        return "k_normals3-TIES"
    h = _holes(elev)
    if route == "scores":
        if h == 0.0:
            return "k_normals3s" if round(c) in (9, 10) else "k_normals3-clean"
        return "k_normals3-sparse" if h <= 0.002 else "k_normals3-dense"
    return "k_normals3-KEEP-dense"


def routes_of(name):
    _, rows, cols, res, pos, elev, over = cc.case(name)
    over, rank = _split(over)
    out = ["kept", "scores", "batch+region"]
    if not rank:  # (the rank rule lives in the generic kernel alone and is refused on the route of any radius)
        out += ["generic", "any"]
        if rows >= 64 and _cells(over, res) < 11:
            out.append("rows48")
    return out


CASES = [pytest.param(n, r, id=f"{n}-{r}-{kernel_of(n, r)}") for n in cc.names() for r in routes_of(n)]


def _fixture(name, route):
    """(rows, cols, res, pos, elev, overrides, rank rule) of the fixture as this route runs it."""
    _, rows, cols, res, pos, elev, over = cc.case(name)
    over, rank = _split(over)
    if route == "rows48":  # the first 48 cells along i: too narrow for the marching kernels
        elev = np.ascontiguousarray(elev.reshape(cols, rows)[:, :48]).reshape(-1)
        rows = 48
    return rows, cols, res, pos, elev, over, rank


_want = {}


def want_of(oracle, name, route, elev=None, tag=""):
    key = (name, "rows48" if route == "rows48" else "", tag)
    if key not in _want:
        rows, cols, res, pos, e, over, rank = _fixture(name, route)
        oracle.set_normals_rank_rule(rank)
        try:
            _want[key] = oracle.chain(oracle.geom(rows, cols, res, pos), oracle.default_params(**over), e if elev is None else elev, want_normals=True)
        finally:
            oracle.set_normals_rank_rule(False)
    return _want[key]


def run(capi, oracle, name, route):
    rows, cols, res, pos, elev, over, rank = _fixture(name, route)
    flags = 0 if route == "scores" else capi.RUN_KEEP_NORMALS
    if route == "generic":
        flags |= capi.RUN_GENERIC_KERNELS
    with capi.Context(0) as ctx:
        if route == "any":
            ctx.set_option(capi.OPT_FILTER_ANY_RADIUS, 2)
        if rank:
            ctx.set_option(capi.OPT_NORMALS_RANK_RULE, 1)
        ctx.set_params(to_te_params(capi, oracle.default_params(**over)))
        ctx.set_geometry(rows, cols, 1, res, pos)
        ctx.upload_elevation(elev)
        ctx.run_chain(flags)
        ctx.sync()
        return {k: ctx.download(k) for k in OUT_LAYERS + (() if route == "scores" else NRM)}


def check(oracle, name, route, got, want, elev, ctx):
    rows, cols, res, pos, _, over, rank = _fixture(name, route)
    op = oracle.default_params(**over)
    got = {k: np.array(v, np.float32).reshape(-1) for k, v in got.items()}  # (the forgiving helper writes into its input)
    for k in OUT_LAYERS:
        d = np.abs(np.asarray(got[k], np.float64).reshape(-1) - np.asarray(want[k], np.float64).reshape(-1))
        print(f"{ctx}: {k} max|d| = {np.nanmax(d) if np.isfinite(d).any() else 0.0:.3g}")
    if not rank:  # (the helper recomputes the oracle's normals without the rule)
        _forgive_rounding_ties_of_the_normal_layer(oracle, got, want, op, rows, cols, res, pos, elev)
    assert_layers_match(got, want, tol=TOL, ctx=ctx)
    for k in OUT_LAYERS:
        assert np.array_equal(np.isnan(np.asarray(got[k]).reshape(-1)), np.isnan(want[k].reshape(-1))), (ctx, k)
    if "surface_normal_z" in got:
        g, w = orient_horizontal_normals(got, want["surface_normal_z"]), orient_horizontal_normals(want, want["surface_normal_z"])
        assert_layers_match(g, w, layers=NRM, tol=NORMALS_TOL, ctx=ctx + " (normals)")


_default = {}


def default_of(capi, oracle, name):
    if name not in _default:
        _default[name] = run(capi, oracle, name, "kept")
    return _default[name]


POISON = np.float32(-7.0)


def batch_and_region(capi, oracle, name):
    """Two copies of the fixture as a batch; then the score layers of map 1 are overwritten on the device and an odd-origin
    rectangle of it is run again as a region.  Only the admitted input itself is judged: both maps of the batch, and after
    the region run every cell of the rectangle, against the fixture's oracle; outside the rectangle a cell either still
    holds the overwritten value or was recomputed (a region run may refresh the cells around it) and then matches too."""
    # (the combined layer: see test_route)
    rows, cols, res, pos, elev, over, rank = _fixture(name, "batch+region")
    r0, c0, h, w = 7, 13, min(71, rows - 9), 97
    n = rows * cols
    with capi.Context(0) as ctx:
        if rank:
            ctx.set_option(capi.OPT_NORMALS_RANK_RULE, 1)
        ctx.set_params(to_te_params(capi, oracle.default_params(**over)))
        ctx.set_geometry(rows, cols, 2, res, pos)
        ctx.upload_elevation(np.concatenate([elev, elev]))
        ctx.run_chain(capi.RUN_KEEP_NORMALS)
        ctx.sync()
        first = [{k: ctx.download(k, b, 1) for k in OUT_LAYERS + NRM} for b in range(2)]
        for k in OUT_LAYERS:
            ctx.upload_layer(k, np.full(n, POISON, np.float32), 1)
        ctx.run_chain_region(1, r0, c0, h, w, capi.RUN_KEEP_NORMALS)
        ctx.sync()
        second = {k: np.asarray(ctx.download(k, 1, 1), np.float32).reshape(cols, rows) for k in OUT_LAYERS}
    inside = np.zeros((cols, rows), bool)
    inside[c0:c0 + w, r0:r0 + h] = True
    return first, second, inside


@pytest.mark.parametrize("name,route", CASES)
def test_route(capi, oracle, threads, name, route):
    """One fixture on one route: the four score layers within TOL of the oracle (rounding ties of the normal layer forgiven
    as in the random sweep, at most 3 cells), equal NaN patterns, the kept normals; and the scores within TOL of the
    default route's."""
    if route == "batch+region":
        first, second, inside = batch_and_region(capi, oracle, name)
        want = want_of(oracle, name, route)
        elev = _fixture(name, route)[4]
        for b in range(2):
            check(oracle, name, route, first[b], want, elev, f"{name}, map {b} of a batch")
        assert_layers_match(first[0], default_of(capi, oracle, name), tol=TOL, ctx=f"{name}: map 0 of a batch against the single map")
        rows, cols = inside.shape[1], inside.shape[0]
        for k in OUT_LAYERS:
            assert not (second[k][inside] == POISON).any(), (name, k, "a cell of the rectangle was not computed")
        # (the combined layer is judged inside the rectangle only: around it a region run combines again what it finds in the
        # three score layers, recomputed or not -- here the overwritten values)
        merged = {k: np.where((second[k] == POISON) | ((k == "traversability") & ~inside), want[k].reshape(cols, rows), second[k]).reshape(-1)
                  for k in OUT_LAYERS}
        check(oracle, name, route, merged, want, elev, f"{name}, region run")
        return
    got = run(capi, oracle, name, route) if route != "kept" else default_of(capi, oracle, name)
    elev = _fixture(name, route)[4]
    check(oracle, name, route, got, want_of(oracle, name, route), elev, f"{name}, {route}")
    if route not in ("kept", "rows48"):  # (the 48-row copy is another map: its border discs differ)
        assert_layers_match(got, default_of(capi, oracle, name), tol=TOL, ctx=f"{name}: {route} against the default route")


def test_rows48_against_the_wide_map(capi, oracle):
    """k_normals_slide on the 48-row copy against the marching kernels on the whole map, on the cells whose discs both maps
    hold entirely (cells of the copy at least R + 1 cells from its cut edge).  (test_route judges the copy against the oracle
    on all of its cells; the copy as a map of its own is not admitted one by one -- its discs away from the cut are the
    admitted fixture's.)"""
    for name in cc.names():
        if "rows48" not in routes_of(name):
            continue
        _, rows, cols, res, pos, elev, over = cc.case(name)
        R = int(np.ceil(_cells(over, res))) + 1
        # the copy is another map geometry (48 cells long along x): tie cells are decided from rounded positions, so only
        # tie-free fixtures can be compared cell by cell
        if abs(_cells(over, res) - round(_cells(over, res))) < 1e-9:
            continue
        narrow = run(capi, oracle, name, "rows48")
        wide = default_of(capi, oracle, name)
        for k in ("traversability_slope", "traversability_roughness"):
            a = np.asarray(narrow[k]).reshape(cols, 48)[:, :48 - R]
            b = np.asarray(wide[k]).reshape(cols, rows)[:, :48 - R]
            assert_layers_match({k: a}, {k: b}, layers=(k,), tol=TOL, ctx=f"{name}: 48-row copy against the whole map")


@pytest.mark.parametrize("name", cc.LONG_STRIP)
@pytest.mark.parametrize("keep", [True, False], ids=["kept", "scores"])
def test_long_strips(capi, oracle, threads, name, keep):
    """LONG_STRIP_MAPS copies of one plane along j as a batch: each map is left 9 to 12 resident slots, so n3_plan_strips cuts
    it into strips of 80 to 319 rows (test_long_strip_batches_get_long_strips asks the plan's code) -- the slid moments run
    that far from their direct sums and |z - zref| grows to 45 .. 160 m inside a strip at res 0.5.  The first, a middle and
    the last map against the fixture's oracle and against the single-map run."""
    rows, cols, res, pos, elev, over, rank = _fixture(name, "kept")
    B = cc.LONG_STRIP_MAPS
    layers = OUT_LAYERS + (NRM if keep else ())
    with capi.Context(0) as ctx:
        ctx.set_params(to_te_params(capi, oracle.default_params(**over)))
        ctx.set_geometry(rows, cols, B, res, pos)
        ctx.upload_elevation(np.tile(elev, B))
        ctx.run_chain(capi.RUN_KEEP_NORMALS if keep else 0)
        ctx.sync()
        got = {b: {k: ctx.download(k, b, 1) for k in layers} for b in (0, B // 2 + 1, B - 1)}
    want = want_of(oracle, name, "kept")
    for b, g in got.items():
        check(oracle, name, "kept", g, want, elev, f"{name}, map {b} of {B}, {'kept' if keep else 'scores'}")
        assert_layers_match(g, default_of(capi, oracle, name), tol=TOL, ctx=f"{name}: map {b} of {B} against the single map")
