"""Parity over the parameters no other GPU test varies (tests/param_route_cases.py): four distinct weights at each of the ten
places that write `traversability`, normal_vector_positive_axis x / y on every kind of run k_normals serves, and fp_max_gap on
whole and region runs with the footprint pass.  tests/test_chain_route.py holds every case to the route it claims,
tests/test_param_routes_ref.py proves the cases' preconditions with the oracle alone.

The weighted sum is the float32 statement of the device's own three score layers bit for bit (-ffp-contract=off);
everything else is the oracle's within the suite's 1e-5 (tests/helpers.py), the step layer bit for bit, NaN patterns exact."""
import numpy as np
import pytest

from tests import param_route_cases as P
from tests.helpers import OUT_LAYERS, TOL, assert_layers_match, orient_axis_normals, to_te_params

pytestmark = pytest.mark.gpu

NRM = ("surface_normal_x", "surface_normal_y", "surface_normal_z")
FP = ("traversability_footprint",)
MEMO = ("slope_footprint", "step_footprint", "roughness_footprint")
SCORES = OUT_LAYERS[:3]


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no MI355X visible"
    return capi


def _ids(cases):
    return ["%s-%s" % (P.case_id(c), "+".join(str(w) for w in c.route if w not in ("none", "-", 0, 1)).replace(" ", "")) for c in cases]


def _bits(a):
    return np.asarray(a, np.float32).reshape(-1).view(np.uint32)


def _flags(capi, c, memo=False):
    return ((capi.RUN_KEEP_NORMALS if c.keep else 0) | (capi.RUN_GENERIC_KERNELS if c.generic and c.kind != "rank" else 0) |
            (capi.RUN_FOOTPRINT if c.footprint else 0) | (capi.RUN_FOOTPRINT_MEMO if memo else 0))


def run(capi, oracle, c, memo=False):
    """-> (device layers, [final maps]): the case's calls through the C-ABI; every layer downloaded whole."""
    maps = P.elevation(c)
    layers = OUT_LAYERS + (NRM if c.keep else ()) + (FP if c.footprint else ()) + (MEMO if memo else ())
    with capi.Context(0) as ctx:
        if c.any_option:
            ctx.set_option(capi.OPT_FILTER_ANY_RADIUS, c.any_option)
        if c.kind == "rank":
            ctx.set_option(capi.OPT_NORMALS_RANK_RULE, 1)
        ctx.set_params(to_te_params(capi, P.params(oracle, c)))
        ctx.set_geometry(c.rows, c.cols, c.batch, c.res, P.POS)
        ctx.upload_elevation(np.stack(maps))
        if c.kind == "filter":
            for f in ("normals", "slope", "roughness"):
                ctx.run_filter(f)
            layers = ("traversability_slope", "traversability_roughness") + NRM
        else:
            ctx.run_chain(_flags(capi, c, memo))
        if c.kind == "region":
            r0, c0, h, w = c.region
            t = P.tile(c, maps[0])
            maps[0][c0:c0 + w, r0:r0 + h] = t
            ctx.upload_tile(t, 0, r0, c0)
            ctx.run_chain_region(0, r0, c0, h, w, flags=_flags(capi, c, memo))
        ctx.sync()
        got = {k: ctx.download(k) for k in layers}
    return got, maps


def want_of(oracle, c, elev, memo=False):
    g, op = oracle.geom(c.rows, c.cols, c.res, P.POS), P.params(oracle, c)
    oracle.set_normals_rank_rule(c.kind == "rank")
    try:
        want = oracle.chain(g, op, elev, want_normals=True)
    finally:
        oracle.set_normals_rank_rule(False)
    if c.footprint:
        fp, m = oracle.footprint(g, op, elev, want, want_memo=True)
        want["traversability_footprint"] = fp
        want.update(m)
    return want


def _map(got, b, n):
    return {k: v[b * n:(b + 1) * n] for k, v in got.items()}


def check_sum_of_own_scores(c, got):
    """traversability is the float32 statement w_scale * ((w_slope * slope + w_step * step) + w_rough * roughness) of the device's
    own score layers: the same NaN cells, every other cell bit for bit."""
    f = np.float32
    w = [f(v) for v in c.weights]
    s, t, r = (np.asarray(got[k], f) for k in SCORES)
    want = w[0] * ((w[1] * s + w[2] * t) + w[3] * r)
    have = got["traversability"]
    assert np.array_equal(np.isnan(have), np.isnan(want)), (c.name, "NaN pattern", np.flatnonzero(np.isnan(have) != np.isnan(want))[:8])
    assert np.array_equal(np.isnan(have), np.isnan(s) | np.isnan(t) | np.isnan(r)), (c.name, "a zero weight hid a NaN")
    ok = ~np.isnan(have)
    bad = np.flatnonzero(_bits(have[ok]) != _bits(want[ok]))
    assert bad.size == 0, (c.name, bad.size, [(float(have[ok][o]), float(want[ok][o])) for o in bad[:5]])
    assert ok.sum() >= 20


@pytest.mark.parametrize("c", P.WEIGHTS, ids=_ids(P.WEIGHTS))
def test_weights_at_every_place_that_combines(capi, oracle, c):
    got, maps = run(capi, oracle, c)
    check_sum_of_own_scores(c, got)
    n = c.rows * c.cols
    for b, e in enumerate(maps):
        want, g = want_of(oracle, c, e), _map(got, b, n)
        what = "%s, map %d" % (c.name, b)
        assert_layers_match(g, want, layers=OUT_LAYERS + (FP if c.footprint else ()), ctx=what)
        assert np.array_equal(_bits(g["traversability_step"]), _bits(want["traversability_step"])), what


@pytest.mark.parametrize("name", sorted(P.WEIGHT_SETS))
def test_combine_plugin_on_layers_with_independent_nans(capi, name):
    """TE_FILTER_COMBINE (k_combine) on uploaded score layers whose NaN cells are independent of each other -- a chain never
    leaves such layers: its step layer is NaN only where slope and roughness are too --, so a term skipped for its zero weight
    (the signed set: w_step = 0) shows as a finite cell where the step layer alone is NaN."""
    rows, cols = 70, 37
    w = P.WEIGHT_SETS[name]
    rng = np.random.default_rng(23)
    layers = [rng.uniform(0.0, 1.0, rows * cols).astype(np.float32) for _ in range(3)]
    for k, a in enumerate(layers):
        a[rng.random(a.size) < 0.1] = k % 2  # the clips
        a[rng.random(a.size) < 0.05] = np.nan
    alone = np.isnan(layers[1]) & ~np.isnan(layers[0]) & ~np.isnan(layers[2])
    assert alone.sum() >= 20
    c = P.WEIGHTS[0]._replace(name="combine plugin, %s weights" % name, weights=w)
    with capi.Context(0) as ctx:
        ctx.set_params(capi.default_params(w_scale=w[0], w_slope=w[1], w_step=w[2], w_rough=w[3]))
        ctx.set_geometry(rows, cols, 1, P.RES, P.POS)
        for k, a in zip(SCORES, layers):
            ctx.upload_layer(k, a)
        ctx.run_filter("combine")
        ctx.sync()
        got = {k: ctx.download(k) for k in OUT_LAYERS}
    for k, a in zip(SCORES, layers):
        assert np.array_equal(_bits(got[k]), _bits(a)), (k, "an input layer changed")
    check_sum_of_own_scores(c, got)
    assert np.isnan(got["traversability"][alone]).all()


def check_axis(oracle, c, elev, got, want, what):
    """Scores, NaN pattern and kept normals of one map against the oracle.  Sign-free cells (tests/param_route_cases.py) are
    compared up to the sign of the whole normal: there the slope score of either sign is accepted, and the weighted sum follows."""
    free = P.sign_free(c, elev, want)
    layers = [k for k in OUT_LAYERS if k in got]
    for k in layers + [k for k in NRM if k in got]:
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), (what, k, "NaN pattern")
    other = dict(want)  # the oracle's layers had rounding gone the other way on the sign-free cells
    other["traversability_slope"] = oracle.slope(oracle.geom(c.rows, c.cols, c.res, P.POS), -want["surface_normal_z"], P.params(oracle, c).slope_critical)
    other["traversability"] = oracle.combine(other["traversability_slope"], want["traversability_step"], want["traversability_roughness"], *c.weights)
    for k in layers:
        d = np.abs(got[k].astype(np.float64) - want[k])
        alt = np.abs(got[k].astype(np.float64) - other[k])
        bad = ~np.isnan(want[k]) & ~((d <= TOL) | (free & (alt <= TOL)))
        assert not bad.any(), (what, k, int(bad.sum()), float(np.nanmax(d)))
    if "traversability_step" in got:
        assert np.array_equal(_bits(got["traversability_step"]), _bits(want["traversability_step"])), what
    if c.keep:
        a, b = orient_axis_normals(got, want, free), orient_axis_normals(want, want, free)
        assert_layers_match(a, b, layers=NRM, tol=1e-5, ctx=what + " (normals)")
        comp = got[NRM[c.axis]]
        assert (comp[~np.isnan(comp)] >= 0).all(), (what, "a normal points against the positive axis")
    assert free.sum() <= 0.002 * max(1, np.isfinite(elev).sum())


@pytest.mark.parametrize("c", P.AXIS, ids=_ids(P.AXIS))
def test_positive_axis_x_and_y(capi, oracle, c):
    got, maps = run(capi, oracle, c)
    if c.kind != "filter":
        check_sum_of_own_scores(c, got)
    n = c.rows * c.cols
    for b, e in enumerate(maps):
        want = want_of(oracle, c, e)
        check_axis(oracle, c, e, _map(got, b, n), want, "%s, map %d" % (c.name, b))
        if c.footprint:
            assert_layers_match(_map(got, b, n), want, layers=FP, ctx=c.name)


@pytest.mark.parametrize("c", P.GAP, ids=_ids(P.GAP))
def test_max_gap_width(capi, oracle, c):
    """Footprint and memo layers against the oracle's from-scratch result at each fp_max_gap; the region case after a tile whose
    box a ray of 20 cells meets from 15 cells outside the tile."""
    got, maps = run(capi, oracle, c, memo=True)
    want = want_of(oracle, c, maps[0])
    assert_layers_match(got, want, layers=list(OUT_LAYERS) + ["traversability_footprint", "slope_footprint", "step_footprint"], ctx=c.name)
    assert (got["traversability_footprint"] == 0).any() and (got["step_footprint"] == 0).any() and (got["step_footprint"] == 1).any()
