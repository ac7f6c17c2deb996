"""te_run_filter, the entry point of the drop-in SlopeFilter / StepFilter / RoughnessFilter / SurfaceNormalsFilter plugins: every
plugin on every route plan_filter_route (te_chain_route.h) can give it, on every cell, against the oracle's single filters --
on layers the plugin did not compute itself.

The cases, their inputs and the route each claims: tests/plugin_filter_cases.py (tests/test_chain_route.py holds every claim
against the library's own plan, without a GPU).  The yardsticks: oracle.slope / step / roughness / normals / combine, which
tests/test_plugin_filter_ref.py holds against oracle.chain and against a numpy restatement.  Tolerances: bit for bit where
DESIGN.md says so (step, combine, untouched layers), the suite's 1e-5 for device against oracle (tests/helpers.py), exact NaN and
zero patterns.  No cell is left out of a comparison."""
import os

import numpy as np
import pytest

from tests import conditioning_cases as cc
from tests import plugin_filter_cases as K
from tests.helpers import OUT_LAYERS, TOL, assert_layers_match, compare_layer, orient_horizontal_normals, to_te_params

pytestmark = pytest.mark.gpu

NRM = ("surface_normal_x", "surface_normal_y", "surface_normal_z")
UNTOUCHED = np.float32(7.25)
SEQUENCE = ("normals", "slope", "step", "roughness", "combine")  # the order of robot_filter_parameter.yaml


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


def _bits(a):
    return np.asarray(a, np.float32).reshape(-1).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _ids(cases):
    return [f"{K.case_id(c)}-{K.route_words(c).replace(' ', '+')}" for c in cases]


def _context(capi, c, op, pos=(0.0, 0.0)):
    ctx = capi.Context(0)
    if c.any_option:
        ctx.set_option(capi.OPT_FILTER_ANY_RADIUS, c.any_option)
    ctx.set_params(to_te_params(capi, op))
    ctx.set_geometry(c.rows, c.cols, c.batch, c.res, pos)
    return ctx


def _flags(capi, c):
    return capi.RUN_GENERIC_KERNELS if c.generic else 0


def _score_cells(layer, got, want, what):
    """One score layer against the oracle's on every cell: NaN pattern, zero pattern, values."""
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    n_bad, worst, _ = compare_layer(layer, got, want, TOL)
    print(f"{what}: {layer} max|d| = {worst:.3g}, {int((want == 0).sum())} zeros, {int(np.isnan(want).sum())} NaN of {want.size}")
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN pattern", np.flatnonzero(np.isnan(got) != np.isnan(want))[:8])
    assert np.array_equal(got == 0, want == 0), (what, "zero / non-zero pattern", np.flatnonzero((got == 0) != (want == 0))[:8])
    assert n_bad == 0, (what, n_bad, worst)


# ---- SlopeFilter on a surface_normal_z it did not compute -------------------------------------------------------------------

@pytest.mark.parametrize("name", ["table", "random", "batch"])
def test_slope_from_foreign_nz(capi, oracle, name):
    """k_slope_from_nz on values no chain writes: the ends of acos' domain and beyond, zeros of both signs, a denormal, the
    critical angle's cosine and its float32 neighbours, NaN and both infinities; and a random layer over [-1, 1]."""
    op = oracle.default_params()
    crit = float(op.slope_critical)
    rows, cols, maps = K.slope_layers(crit)[name]
    nz = np.concatenate(maps)
    with capi.Context(0) as ctx:
        ctx.set_params(to_te_params(capi, op))
        ctx.set_geometry(rows, cols, len(maps), K.RES)
        ctx.upload_layer("surface_normal_z", nz)
        ctx.run_filter("slope")
        ctx.sync()
        got = [ctx.download("traversability_slope", b, 1) for b in range(len(maps))]
        assert _same_bits(ctx.download("surface_normal_z"), nz), "the input layer changed"
    g = oracle.geom(rows, cols, K.RES)
    for b, (z, s) in enumerate(zip(maps, got)):
        want = oracle.slope(g, z, crit)
        _score_cells("traversability_slope", s, want, f"slope of {name}, map {b}")
        assert np.array_equal(np.isnan(s), ~np.isfinite(z))
        beyond = np.isfinite(z) & (np.abs(z) > 1.0)
        assert (s[z == 1.0] == 1.0).all() and (s[beyond] == 0.0).all() and (s[z == -1.0] == 0.0).all()
    if name == "table":  # (every value of the table is in the layer, the three cells at the threshold on both sides of it)
        k = got[0][9:12]
        assert np.isin(_bits(K.slope_values(crit)), _bits(maps[0])).all() and (k == 0).any() and (k > 0).any()


# ---- StepFilter alone ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", K.STEP, ids=_ids(K.STEP))
def test_step_alone(capi, oracle, c):
    """traversability_step of te_run_filter(step) is the oracle's bit for bit on every step route, on maps
    with 2 % speckle and an unobserved block; each map of a batch against its own oracle result."""
    maps = K.elevation(c)
    op = oracle.default_params(step_radius1=K.radius(c, 0), step_radius2=K.radius(c, 1))
    with _context(capi, c, op) as ctx:
        ctx.upload_elevation(np.concatenate(maps))
        ctx.run_filter("step", _flags(capi, c))
        ctx.sync()
        got = [ctx.download("traversability_step", b, 1) for b in range(c.batch)]
        assert _same_bits(ctx.download("elevation"), np.concatenate(maps)), "the elevation changed"
    g = oracle.geom(c.rows, c.cols, c.res)
    for b, (e, s) in enumerate(zip(maps, got)):
        want = oracle.step(g, e, op.step_critical, op.step_radius1, op.step_radius2, op.step_ncrit)
        bad = np.flatnonzero(_bits(s) != _bits(want))
        assert bad.size == 0, (K.case_id(c), b, [(int(o % c.rows), int(o // c.rows), float(s[o]), float(want[o])) for o in bad[:6]])
        if not np.isfinite(e).any():
            assert np.isnan(s).all()
        elif 0 < max(c.cells) < 10 and min(c.rows, c.cols) > 8 and b == (1 if c.batch == 3 else 0):  # (the input is not a trivial one: scores on both sides and between)
            assert ((want > 0) & (want < 1)).sum() > 20 and (want == 1).any(), K.case_id(c)


# ---- RoughnessFilter with the normals it is given -----------------------------------------------------------------------------

def _critical_values(oracle, g, elev, nrm, radius):
    """The default critical value, and two placed on a cell's own roughness at the 30 % and 70 % quantile of the oracle's
    (tests/test_gpu_round5.py: the cell's float32 score turned back into a roughness, so the cell lies within a float32 ulp of
    the threshold and far outside the rounding of a double sum).  None where fewer than ten cells have a positive roughness."""
    out = [0.05]
    coarse = (1.0 - oracle.roughness(g, elev, *nrm, 10.0, radius).astype(np.float64)) * 10.0
    some = coarse[np.isfinite(coarse) & (coarse > 1e-3) & (coarse < 5.0)]
    if some.size < 10:
        return out
    for q in (0.3, 0.7):
        twice = 2.0 * float(np.quantile(some, q))
        fine = (1.0 - oracle.roughness(g, elev, *nrm, twice, radius).astype(np.float64)) * twice
        idx = np.flatnonzero(np.isfinite(fine) & (fine > 1e-3) & (fine < twice))
        out.append(float(fine[idx[np.argmin(np.abs(fine[idx] - 0.5 * twice))]]))  # (the cell nearest the quantile)
    return out


@pytest.mark.parametrize("c", K.ROUGHNESS, ids=_ids(K.ROUGHNESS))
def test_roughness_with_given_normals(capi, oracle, threads, c):
    """te_run_filter(roughness) on every roughness route x every kind of normal layer (tests/plugin_filter_cases.py), each at the
    default critical value and at two placed on a cell's own roughness: NaN exactly where surface_normal_x is NaN, the oracle's
    zeros, values within 1e-5; the four input layers keep their bits and the other score layers are not written."""
    g = oracle.geom(c.rows, c.cols, c.res)
    radius = K.radius(c)
    per, n_runs = c.rows * c.cols, 0
    with _context(capi, c, oracle.default_params(rough_radius=radius)) as ctx:
        for kind in K.NORMAL_KINDS:
            maps = K.elevation(c, kind=kind)
            nrm = [K.normals(kind, e, lambda e=e: oracle.normals(g, e, radius), 7 + b) for b, e in enumerate(maps)]
            layers = [np.concatenate([n[k] for n in nrm]) for k in range(3)]
            main = 1 if c.batch == 3 else 0
            for crit in _critical_values(oracle, g, maps[main], nrm[main], radius):
                what = f"{K.case_id(c)}, {kind} normals, critical value {crit!r}"
                ctx.set_params(to_te_params(capi, oracle.default_params(rough_radius=radius, rough_critical=crit)))
                ctx.upload_elevation(np.concatenate(maps))
                for k, a in zip(NRM, layers):
                    ctx.upload_layer(k, a)
                for k in ("traversability_slope", "traversability_step"):
                    ctx.upload_layer(k, np.full(per * c.batch, UNTOUCHED, np.float32))
                ctx.run_filter("roughness", _flags(capi, c))
                ctx.sync()
                got = [ctx.download("traversability_roughness", b, 1) for b in range(c.batch)]
                for k, a in zip(NRM, layers):
                    assert _same_bits(ctx.download(k), a), (what, k, "an input layer changed")
                assert _same_bits(ctx.download("elevation"), np.concatenate(maps)), (what, "the elevation changed")
                for k in ("traversability_slope", "traversability_step"):
                    assert (ctx.download(k) == UNTOUCHED).all(), (what, k, "was written")
                for b in range(c.batch):
                    want = oracle.roughness(g, maps[b], *nrm[b], crit, radius)
                    _score_cells("traversability_roughness", got[b], want, f"{what}, map {b}")
                    assert np.array_equal(np.isnan(got[b]), ~np.isfinite(nrm[b][0]))
                    if not np.isfinite(maps[b]).any():
                        assert np.isnan(got[b]).all()
                    elif crit != 0.05 and b == main and per >= 1000:  # (placed inside the distribution: both sides are populated)
                        assert (want == 0).sum() > per // 8 and (want > 0).sum() > per // 8, what
                n_runs += 1
            if kind == "void":  # windows without a point score 1, windows of one point 0, all under valid normals
                w = oracle.roughness(g, maps[main], *nrm[main], 0.05, radius)
                assert (w == 1.0).any() and (w[np.isfinite(maps[main])] == 0.0).all()
    assert n_runs >= len(K.NORMAL_KINDS) + 2 * 5  # (at least five kinds had a distribution to place critical values in)


# ---- SurfaceNormalsFilter alone, then the plugins in the reference's order -----------------------------------------------------

def _five_calls(capi, ctx, flags=0):
    for f in SEQUENCE:
        ctx.run_filter(f, flags)
    ctx.sync()
    return {k: ctx.download(k) for k in OUT_LAYERS + NRM}


def _combine_of_own_scores(oracle, op, got):
    return oracle.combine(got["traversability_slope"], got["traversability_step"], got["traversability_roughness"], op.w_scale, op.w_slope,
                          op.w_step, op.w_rough)


@pytest.mark.parametrize("c", K.NORMALS, ids=_ids(K.NORMALS))
def test_normals_alone_then_the_plugins_in_order(capi, oracle, c):
    """TE_FILTER_NORMALS on each of its routes, then SLOPE, STEP, ROUGHNESS and COMBINE on the layers it left: the chain of the
    unchanged YAML, one plugin at a time, against oracle.chain; the combined layer is the weighted sum of the device's own three
    scores bit for bit."""
    elev = K.elevation(c)[0]
    r = K.radius(c)
    op = oracle.default_params(normals_radius=r, rough_radius=r, step_radius1=2.5 * c.res, step_radius2=2.5 * c.res)
    want = oracle.chain(oracle.geom(c.rows, c.cols, c.res), op, elev, want_normals=True)
    with _context(capi, c, op) as ctx:
        ctx.upload_elevation(elev)
        got = _five_calls(capi, ctx, _flags(capi, c))
    assert_layers_match(got, want, ctx=K.case_id(c))
    for k in OUT_LAYERS + NRM:
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), (K.case_id(c), k)
    assert _same_bits(got["traversability_step"], want["traversability_step"])
    g, w = orient_horizontal_normals(got, want["surface_normal_z"]), orient_horizontal_normals(want, want["surface_normal_z"])
    assert_layers_match(g, w, layers=NRM, tol=TOL, ctx=K.case_id(c) + " (normals)")
    assert _same_bits(got["traversability"], _combine_of_own_scores(oracle, op, got))


# ---- hard conditioning on the plugin path ---------------------------------------------------------------------------------------

CONDITIONING = [n for n in cc.names() if cc.case(n)[1] >= 64]  # (the marches need 64 rows; the 48-row fixtures are the chain's)
FOREIGN = [n for n in CONDITIONING if "alt" in n or "res0.5" in n]


@pytest.mark.parametrize("name", CONDITIONING)
def test_conditioning_fixture_one_plugin_at_a_time(capi, oracle, threads, name):
    """The fixtures of tests/conditioning_cases.py -- altitude, relief, resolutions far from 0.05 m, a far map origin, the rank rule
    -- through the five single-plugin calls, judged exactly as tests/test_gpu_conditioning.py judges the chain."""
    from tests.test_gpu_conditioning import _fixture, check, want_of
    rows, cols, res, pos, elev, over, rank = _fixture(name, "kept")
    op = oracle.default_params(**over)
    with capi.Context(0) as ctx:
        if rank:
            ctx.set_option(capi.OPT_NORMALS_RANK_RULE, 1)
        ctx.set_params(to_te_params(capi, op))
        ctx.set_geometry(rows, cols, 1, res, pos)
        ctx.upload_elevation(elev)
        got = _five_calls(capi, ctx)
    assert _same_bits(got["traversability"], _combine_of_own_scores(oracle, op, got))
    check(oracle, name, "kept", got, want_of(oracle, name, "kept"), elev, f"{name}, one plugin at a time")


@pytest.mark.parametrize("name", FOREIGN)
def test_conditioning_fixture_roughness_of_foreign_normals(capi, oracle, threads, name):
    """The closed form n^T C n of the given-normals roughness with a normal that is not the disc's eigenvector, where the
    moments cancel: the altitude and res-0.5 fixtures with tilted foreign normals against oracle.roughness on every cell, at the
    fixture's own critical value and at one as large as the radius (tilted normals are rough: most scores are non-zero there)."""
    from tests.test_gpu_conditioning import _fixture
    rows, cols, res, pos, elev, over, rank = _fixture(name, "kept")
    op = oracle.default_params(**over)
    g = oracle.geom(rows, cols, res, pos)
    nrm = K.normals("tilted", elev, None, 99)
    with capi.Context(0) as ctx:
        ctx.set_geometry(rows, cols, 1, res, pos)
        for crit in (float(op.rough_critical), float(op.rough_radius)):
            op.rough_critical = crit
            ctx.set_params(to_te_params(capi, op))
            ctx.upload_elevation(elev)
            for k, a in zip(NRM, nrm):
                ctx.upload_layer(k, a)
            ctx.run_filter("roughness")
            ctx.sync()
            got = ctx.download("traversability_roughness")
            want = oracle.roughness(g, elev, *nrm, crit, op.rough_radius)
            _score_cells("traversability_roughness", got, want, f"{name}, tilted normals, critical value {crit!r}")
        assert (want > 0).sum() > rows * cols // 2, name
