"""te_run_expression on the device, through capi, against the independent numpy evaluator tests/ref_py/expression_ref.py:
arithmetic bit for bit at the shapes where the 16-byte groups, the tail and the batch phases can go wrong; reductions per map
(min / max / count exact, sums within one float32 ulp of the float64 sum, the same bits run after run); the transcendental
functions within a measured ulp bound; the shipped expression against the chain's own combine and the bag's layer; the state of
the context afterwards; the refusals."""
import numpy as np
import pytest

from tests.helpers import assert_layers_match, to_te_params
from tests.ref_py import expression_ref as R

pytestmark = pytest.mark.gpu

A, B, C = "traversability_slope", "traversability_step", "traversability_roughness"
SHIPPED = f"(1.0 / 3.0) * ({A} + {B} + {C})"
MIN3 = f"cwiseMin(cwiseMin({A}, {B}), {C})"
# 8 operands on the stack (15 instructions), then 11 x (.* layer + layer) of 4 instructions each, and one abs: 60
LONG = "abs((" + (A + " + (") * 7 + A + ")" * 7 + ")" + f" .* {B} + {C}" * 11 + ")"
EXPRESSIONS = [SHIPPED, MIN3, f"{A} .* {B} - 0.25 * elevation / (1.0 + abs(elevation))", "cwiseMax(traversability - 0.5, 0.0)", LONG]
INPUTS = ("elevation", A, B, C, "traversability")


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    return capi


def random_layers(shape, seed, names=INPUTS, lo=-0.2, hi=1.2, invalid=True):
    """[batch, cols * rows] values with 5 % NaN and 1 % +-inf."""
    rng = np.random.default_rng(seed)
    out = {}
    for name in names:
        x = rng.uniform(lo, hi, size=shape).astype(np.float32)
        if invalid:
            x[rng.random(shape) < 0.05] = np.nan
            x[rng.random(shape) < 0.005] = np.inf
            x[rng.random(shape) < 0.005] = -np.inf
        out[name] = x
    return out


def context(capi, rows, cols, batch, layers):
    ctx = capi.Context(0)
    ctx.set_geometry(rows, cols, batch, 0.1)
    for name, x in layers.items():
        ctx.upload_layer(name, x)
    return ctx


def test_the_long_expression_is_at_the_limits(capi):
    info = capi.expr_check(LONG)
    assert info["n_instructions"] == 60 and info["stack_depth"] == 8 and info["layers"] == [A, B, C], info
    assert capi.expr_check(SHIPPED) == {"n_instructions": 7, "layers": [A, B, C], "n_reductions": 0, "stack_depth": 3}


# cells mod 4 = 1, 3, 3, 3, 0, 0, 1; 67 x 131 is more than one block; 33 x 17 x 3: every map at another 16-byte phase
@pytest.mark.parametrize("rows,cols,batch", [(1, 1, 1), (1, 7, 1), (7, 1, 1), (5, 3, 1), (2, 2, 1), (64, 64, 1), (67, 131, 1), (33, 17, 3)])
def test_arithmetic_is_bit_identical_to_the_reference(capi, rows, cols, batch):
    layers = random_layers((batch, rows * cols), 1000 * rows + cols)
    with context(capi, rows, cols, batch, layers) as ctx:
        for text in EXPRESSIONS:
            ctx.upload_layer("traversability", layers["traversability"])  # (the in-place expression reads it)
            ctx.run_expression(text)
            got = ctx.download("traversability").reshape(batch, -1)
            want = R.evaluate(text, layers)
            assert R.same_bits(got, want), (text[:50], (rows, cols, batch), np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:8])
            # every other layer is as it was
            assert R.same_bits(ctx.download(A).reshape(batch, -1), layers[A])


REDUCE_SHAPES = [(67, 131, 1), (300, 257, 1), (33, 17, 3)]  # 300 x 257: 76 partials per reduction, more than the 64 the finishing workgroup starts from


@pytest.mark.parametrize("rows,cols,batch", REDUCE_SHAPES)
def test_reductions_min_max_and_count_are_exact(capi, rows, cols, batch):
    layers = random_layers((batch, rows * cols), 7 * rows + cols, names=("elevation", A))
    if batch > 1:
        layers["elevation"][1, :] = np.nan  # a map of the batch without a finite cell
        layers["elevation"][2, :] += 3.0    # per-map results differ
    x = "elevation"
    texts = [f"({x} - minOfFinites({x})) / (maxOfFinites({x}) - minOfFinites({x}))", f"numberOfFinites({x}) + 0 * {A}",
             f"maxOfFinites({x} .* {A}) - cwiseMin({A}, minOfFinites(abs({x})))", f"numberOfFinites({x}) - numberOfFinites({A}) + maxOfFinites({A}) * minOfFinites({x})"]
    with context(capi, rows, cols, batch, layers) as ctx:
        for text in texts:
            ctx.run_expression(text)
            got = ctx.download("traversability").reshape(batch, -1)
            assert R.same_bits(got, R.evaluate(text, layers)), (text, (rows, cols, batch))
        if batch > 1:
            for name, want in (("minOfFinites", np.nan), ("maxOfFinites", np.nan), ("meanOfFinites", np.nan), ("sumOfFinites", 0.0), ("numberOfFinites", 0.0)):
                ctx.run_expression(f"{name}({x})")
                got = ctx.download("traversability").reshape(batch, -1)
                assert R.same_bits(got[1], np.full(rows * cols, want, np.float32)), name
                assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all() and got[0, 0] != got[2, 0], name


@pytest.mark.parametrize("rows,cols,batch", REDUCE_SHAPES)
def test_sums_land_within_one_ulp_and_repeat_bit_for_bit(capi, rows, cols, batch):
    """Positive inputs: the double accumulation of at most 8e4 terms errs by under 1e-11 relative, so only the final rounding to
    float32 can differ from the float64 reference -- one ulp.  Subtracted from a layer the difference is no longer one ulp of
    the result, so the scalars are read on their own."""
    layers = random_layers((batch, rows * cols), 11 * rows + cols, names=("elevation", A), lo=0.01, hi=2.0, invalid=False)
    finite_only = {k: v.copy() for k, v in layers.items()}
    finite_only["elevation"][np.random.default_rng(5).random(layers["elevation"].shape) < 0.05] = np.nan
    with context(capi, rows, cols, batch, layers) as ctx:
        for text, data in ((f"sum(elevation)", layers), ("mean(elevation)", layers), (f"mean(elevation .* {A})", layers), (f"sum(sqrt({A}))", layers),
                           ("meanOfFinites(elevation)", finite_only), ("sumOfFinites(elevation)", finite_only)):
            ctx.upload_layer("elevation", data["elevation"])
            ctx.run_expression(text)
            got = ctx.download("traversability").reshape(batch, -1)
            ctx.run_expression(text)
            again = ctx.download("traversability").reshape(batch, -1)
            want = R.evaluate(text, data)
            d = R.ulp_distance(got, want)
            print(f"{text} {rows}x{cols}x{batch}: {d} ulp")
            assert d <= 1, (text, d)
            assert R.same_bits(got, again), text
            assert (got == got[:, :1]).all()  # one scalar per map, broadcast
        # the use the issue names: a layer minus its mean -- the scalar is the one read above
        ctx.upload_layer("elevation", finite_only["elevation"])
        ctx.run_expression("meanOfFinites(elevation)")
        mean = ctx.download("traversability").reshape(batch, -1)[:, :1]
        ctx.run_expression("elevation - meanOfFinites(elevation)")
        got = ctx.download("traversability").reshape(batch, -1)
        assert R.same_bits(got, finite_only["elevation"] - mean)


# Largest distance to float32(f(float64(x))) measured on the MI355X over this test's arguments (printed by the test); the bound
# is twice that, rounded up, and at least 2 ulp.  Above 8 ulp a function is not rounding any more: refused outright.
MEASURED_ULP = {"exp": 1, "log": 2, "log10": 2, "sin": 1, "cos": 1, "tan": 2, "asin": 2, "acos": 1, "^0.5": 1, "^2": 1, "^-1": 1}


def transcendental_cases():
    rng = np.random.default_rng(77)
    n = 4099
    wide = rng.uniform(-20.0, 20.0, n).astype(np.float32)
    unit = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    pos = np.exp(rng.uniform(-20.0, 20.0, n)).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 2.0, -2.0, 0.5], dtype=np.float32)
    cases = {"exp": wide, "log": pos, "log10": pos, "sin": wide, "cos": wide, "tan": wide, "asin": unit, "acos": unit, "^0.5": pos, "^2": wide, "^-1": wide}
    return {k: np.concatenate([special, v]) for k, v in cases.items()}


@pytest.mark.parametrize("fn", list(MEASURED_ULP))
def test_transcendental_functions_within_the_measured_bound(capi, fn):
    x = transcendental_cases()[fn]
    text = f"elevation {fn}" if fn.startswith("^") else f"{fn}(elevation)"
    layers = {"elevation": x.reshape(1, -1)}
    with context(capi, x.size, 1, 1, layers) as ctx:
        ctx.run_expression(text)
        got = ctx.download("traversability").reshape(1, -1)
    want = R.evaluate(text, layers)
    # NaN and the domain errors (log(-1), acos(2), sqrt of a negative) are NaN on both sides
    assert np.array_equal(np.isnan(got), np.isnan(want)), (fn, x[np.isnan(got[0]) != np.isnan(want[0])][:8])
    assert np.isnan(got[0, 0])
    d = R.ulp_distance(got, want)
    print(f"{fn}: max {d} ulp over {x.size} arguments")
    assert d <= 8, (fn, d)
    assert d <= max(2, 2 * MEASURED_ULP[fn]), (fn, d)


def test_the_shipped_expression_is_the_chains_own_combine(capi, bag):
    """Default parameters on the bag map.  The chain's two exactly planar border discs differ from the 2018 filter that wrote the
    bag (test_gpu_chain.py: test_bag_golden_vector_every_cell_with_the_2018_plane_rule), so the golden layer is met under
    TE_OPT_NORMALS_RANK_RULE, the option that reproduces the bag's scores bit for bit; the expression equals the chain's own
    combine either way."""
    rows, cols = int(bag["rows"]), int(bag["cols"])
    with capi.Context(0) as ctx:
        ctx.set_params(capi.default_params())
        ctx.set_geometry(rows, cols, 1, float(bag["resolution"]), tuple(bag["position"]))
        ctx.upload_elevation(bag["elevation"])
        for rank_rule in (0, 1):
            ctx.set_option(capi.OPT_NORMALS_RANK_RULE, rank_rule)
            ctx.run_chain()
            chain = ctx.download("traversability")
            ctx.upload_layer("traversability", np.zeros(rows * cols, np.float32))
            ctx.run_expression(SHIPPED)
            got = ctx.download("traversability")
            assert R.same_bits(got, chain), rank_rule
        assert R.same_bits(got, bag["traversability"])
        assert R.same_bits(chain, bag["traversability"])


def test_the_context_afterwards_is_what_an_upload_leaves(capi, oracle):
    from traversability_estimation_amd import synth
    rows, cols, res = 96, 80, 0.05
    elev = synth.with_steps(synth.perlin_elevation(rows, cols, seed=61, amplitude=0.12), 8, seed=62)
    elev[20:26, 30:41] = np.nan
    op = oracle.default_params()
    g = oracle.geom(rows, cols, res, (0.0, 0.0))
    want = oracle.chain(g, op, elev)
    plain_fp = oracle.footprint(g, op, elev, want)
    scores = {k: np.asarray(want[k], np.float32).reshape(1, -1) for k in (A, B, C)}
    with_min = dict(want)
    with_min["traversability"] = R.evaluate(MIN3, scores).reshape(-1)
    want_fp = oracle.footprint(g, op, elev, with_min)
    p = to_te_params(capi, op)
    with capi.Context(0) as ctx, capi.Context(0) as other:
        for c in (ctx, other):
            c.set_params(p)
            c.set_geometry(rows, cols, 1, res)
            c.upload_elevation(elev)
            c.run_chain()
        before = bytes(capi.params_to_bytes(ctx.get_params()))
        ctx.run_expression(MIN3)
        trav = ctx.download("traversability")
        gpu_scores = {k: ctx.download(k).reshape(1, -1) for k in (A, B, C)}
        assert R.same_bits(trav, R.evaluate(MIN3, gpu_scores).reshape(-1))
        ctx.run_footprint()
        fp = ctx.download("traversability_footprint")
        assert_layers_match({"traversability_footprint": fp}, {"traversability_footprint": want_fp}, layers=["traversability_footprint"], ctx="min-of-three footprint")
        assert not R.same_bits(fp, np.asarray(plain_fp, np.float32).reshape(-1))  # (the expression does change the result here)
        # ... bit for bit what a context that was handed the same values computes
        other.upload_layer("traversability", trav)
        other.run_footprint()
        assert R.same_bits(fp, other.download("traversability_footprint"))
        assert bytes(capi.params_to_bytes(ctx.get_params())) == before
        # the path checks see the new layer (the footprint pass is complete)
        safe, value, status = ctx.check_footprint_paths([np.array([[0.0, 0.0]])])
        assert status[0] == 0
        # the next chain writes the weighted sum again
        ctx.run_chain(capi.RUN_FOOTPRINT)
        other.run_chain(capi.RUN_FOOTPRINT)
        for name in ("traversability", "traversability_footprint"):
            assert R.same_bits(ctx.download(name), other.download(name)), name
        assert_layers_match({"traversability": ctx.download("traversability"), "traversability_footprint": ctx.download("traversability_footprint")},
                            {"traversability": want["traversability"], "traversability_footprint": plain_fp}, layers=["traversability", "traversability_footprint"],
                            ctx="plain chain after an expression")


def test_refusals_leave_the_layer_untouched(capi):
    rows, cols = 21, 13
    layers = random_layers((1, rows * cols), 9)
    with capi.Context(0) as ctx:
        with pytest.raises(capi.TeError) as e:
            ctx.run_expression(SHIPPED)
        assert e.value.code == capi.TE_ERR_NOT_READY and "geometry" in str(e.value)
        ctx.set_params(capi.default_params())
        ctx.set_geometry(rows, cols, 1, 0.1)
        for name, x in layers.items():
            ctx.upload_layer(name, x)

        def refused(text, code, out="traversability"):
            with pytest.raises(capi.TeError) as e:
                ctx.run_expression(text, out)
            assert e.value.code == code, (text, e.value)
            assert R.same_bits(ctx.download("traversability").reshape(1, -1), layers["traversability"]), text
            return str(e.value)

        assert "surface_normal_z" in refused("acos(surface_normal_z)", capi.TE_ERR_NOT_READY)
        refused("slope_footprint + 1", capi.TE_ERR_NOT_READY)
        refused("traversability_x", capi.TE_ERR_NOT_READY)
        refused("robot_slope", capi.TE_ERR_NOT_READY)
        refused(SHIPPED, capi.TE_ERR_INVALID_ARG, out="elevation")
        assert ".*" in refused(f"{A} * {B}", capi.TE_ERR_UNSUPPORTED)
        assert "column" in refused(f"{A} +", capi.TE_ERR_BAD_PARAM)
        # the normals exist with TE_RUN_KEEP_NORMALS, and are gone again after a chain without it
        ctx.upload_elevation(np.zeros(rows * cols, np.float32))
        ctx.run_chain(capi.RUN_KEEP_NORMALS)
        ctx.run_expression("acos(surface_normal_z)")
        got = ctx.download("traversability")
        assert np.nanmax(np.abs(got)) < 1e-3  # a flat map: the normal is +z wherever it exists
        ctx.run_chain()
        with pytest.raises(capi.TeError) as e:
            ctx.run_expression("acos(surface_normal_z)")
        assert e.value.code == capi.TE_ERR_NOT_READY
        # the memo layers exist after a footprint pass, an uploaded optional layer at once
        ctx.run_footprint()
        ctx.run_expression("slope_footprint + step_footprint")
        ctx.upload_layer("robot_slope", layers[A])
        ctx.run_expression("robot_slope * 2")
        assert R.same_bits(ctx.download("traversability").reshape(1, -1), layers[A] * np.float32(2))
