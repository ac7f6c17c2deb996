"""Filters at any radius (TE_OPT_FILTER_ANY_RADIUS, te_filter_any.hip): normals, roughness and step discs beyond 32 cells
through the C-ABI against the oracle, the option's own rules, and the route forced on small discs (option 2) against the
oracle and the default route."""
import os

import numpy as np
import pytest

from tests.helpers import OUT_LAYERS, assert_layers_match, orient_horizontal_normals, to_te_params

pytestmark = pytest.mark.gpu

NRM = ("surface_normal_x", "surface_normal_y", "surface_normal_z")
ERR_UNSUPPORTED = -6


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


def terrain(rows, cols, seed, holes=0.003, block=False, boxes=10, amplitude=0.15):
    from traversability_estimation_amd import synth
    e = synth.with_steps(synth.perlin_elevation(rows, cols, seed=seed, amplitude=amplitude), boxes, seed=seed + 1)
    e = np.array(synth.with_holes(e, holes, seed=seed + 2), np.float32).reshape(cols, rows)
    if block:  # one unobserved region
        e[cols // 3:cols // 3 + 25, rows // 4:rows // 4 + 35] = np.nan
    return e.reshape(-1)


def radii(res, normals, rough, step1, step2):
    return dict(normals_radius=normals * res, rough_radius=rough * res, step_radius1=step1 * res, step_radius2=step2 * res)


def run(capi, op, elev, rows, cols, res, pos=(0.0, 0.0), option=1, flags=0):
    with capi.Context(0) as ctx:
        ctx.set_option(capi.OPT_FILTER_ANY_RADIUS, option)
        ctx.set_params(to_te_params(capi, op))
        ctx.set_geometry(rows, cols, 1, res, pos)
        ctx.upload_elevation(elev)
        ctx.run_chain(flags | capi.RUN_KEEP_NORMALS)
        ctx.sync()
        return {k: ctx.download(k) for k in OUT_LAYERS + NRM}


def want_of(oracle, op, elev, rows, cols, res, pos=(0.0, 0.0)):
    return oracle.chain(oracle.geom(rows, cols, res, pos), op, elev, want_normals=True)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def check(got, want, ctx, normals_tol=1e-5):
    assert_layers_match(got, want, ctx=ctx)
    assert same_bits(got["traversability_step"], want["traversability_step"]), ctx  # max / min / counts: exact
    g, w = orient_horizontal_normals(got, want["surface_normal_z"]), orient_horizontal_normals(want, want["surface_normal_z"])
    assert_layers_match(g, w, layers=NRM, tol=normals_tol, ctx=ctx + " (normals)")


def test_option_rules(capi, oracle):
    """0 refuses a 40-cell disc as before, 1 takes it; going back to 0 while it is held is refused and leaves 1 in force."""
    rows, cols, res = 120, 100, 0.01
    elev = terrain(rows, cols, seed=7001)
    op = oracle.default_params(**radii(res, 40, 40, 3, 3))
    with capi.Context(0) as ctx:
        ctx.set_geometry(rows, cols, 1, res)
        with pytest.raises(capi.TeError) as e:
            ctx.set_params(to_te_params(capi, op))
        assert e.value.code == ERR_UNSUPPORTED
        for bad in (-1, 3):
            with pytest.raises(capi.TeError):
                ctx.set_option(capi.OPT_FILTER_ANY_RADIUS, bad)
        ctx.set_option(capi.OPT_FILTER_ANY_RADIUS, 1)
        ctx.set_params(to_te_params(capi, op))
        with pytest.raises(capi.TeError) as e:
            ctx.set_option(capi.OPT_FILTER_ANY_RADIUS, 0)
        assert e.value.code == ERR_UNSUPPORTED
        ctx.upload_elevation(elev)
        ctx.run_chain(capi.RUN_KEEP_NORMALS)  # (still option 1: the 40-cell discs are served)
        ctx.sync()
        got = {k: ctx.download(k) for k in OUT_LAYERS + NRM}
    check(got, want_of(oracle, op, elev, rows, cols, res), "option 1 kept")


@pytest.mark.parametrize("block", [False, True], ids=["scattered holes", "unobserved block"])
def test_whole_chain_40(capi, oracle, threads, block):
    rows, cols, res, pos = 256, 200, 0.01, (0.37, -1.21)
    elev = terrain(rows, cols, seed=7100 + block, block=block)
    op = oracle.default_params(**radii(res, 40.3, 40.3, 35.2, 40.3))
    check(run(capi, op, elev, rows, cols, res, pos), want_of(oracle, op, elev, rows, cols, res, pos), f"40 cells, block={block}")


@pytest.mark.parametrize("cells,size", [(40.0, (150, 140)), (65.0, (150, 144))], ids=["40 whole", "65: 36 ties"])
def test_tie_radii(capi, oracle, threads, cells, size):
    rows, cols = size
    res, pos = 0.01, (0.013, -0.007)
    elev = terrain(rows, cols, seed=7200 + int(cells))
    op = oracle.default_params(**radii(res, cells, cells, cells, cells))
    check(run(capi, op, elev, rows, cols, res, pos), want_of(oracle, op, elev, rows, cols, res, pos), f"tie radius {cells}")


def test_disc_larger_than_map(capi, oracle, threads):
    rows, cols, res = 40, 520, 0.02
    elev = terrain(rows, cols, seed=7300, boxes=6)
    op = oracle.default_params(**radii(res, 200.2, 200.2, 200.2, 60.5))
    check(run(capi, op, elev, rows, cols, res), want_of(oracle, op, elev, rows, cols, res), "200 cells on 40 x 520")


@pytest.mark.parametrize("case", ["normals 9, roughness 40", "normals 40, roughness 9", "step 40, normals 3", "axis x"])
def test_mixed_sizes(capi, oracle, threads, case):
    """A stage without a large disc keeps its route: bit-identical to a run without the option whose large radius is small."""
    rows, cols, res = 220, 180, 0.01
    elev = terrain(rows, cols, seed=7400, block=True)
    big, small, extra, kept = {
        "normals 9, roughness 40": (radii(res, 9.2, 40.3, 3.3, 3.3), radii(res, 9.2, 9.2, 3.3, 3.3), {}, ("traversability_step",)),
        "normals 40, roughness 9": (radii(res, 40.3, 9.2, 3.3, 3.3), radii(res, 9.2, 9.2, 3.3, 3.3), {}, ("traversability_step",)),
        "step 40, normals 3": (radii(res, 3.3, 3.3, 40.3, 35.2), radii(res, 3.3, 3.3, 3.3, 3.3), {},
                               ("traversability_slope", "traversability_roughness") + NRM),
        "axis x": (radii(res, 40.3, 40.3, 9.2, 9.2), radii(res, 9.2, 9.2, 9.2, 9.2), dict(normals_axis=0), ("traversability_step",)),
    }[case]
    op = oracle.default_params(**big, **extra)
    got = run(capi, op, elev, rows, cols, res)
    check(got, want_of(oracle, op, elev, rows, cols, res), case)
    ref = run(capi, oracle.default_params(**small, **extra), elev, rows, cols, res, option=0)
    for k in kept:
        assert same_bits(got[k], ref[k]), (case, k)


def test_plugin_entry_points(capi, oracle, threads):
    """te_run_filter at 40 cells: STEP, ROUGHNESS with the uploaded normals, NORMALS."""
    rows, cols, res = 200, 170, 0.01
    elev = terrain(rows, cols, seed=7500, block=True)
    op = oracle.default_params(**radii(res, 33.5, 41.2, 40.3, 38.1))
    want = want_of(oracle, op, elev, rows, cols, res)
    with capi.Context(0) as ctx:
        ctx.set_option(capi.OPT_FILTER_ANY_RADIUS, 1)
        ctx.set_params(to_te_params(capi, op))
        ctx.set_geometry(rows, cols, 1, res)
        ctx.upload_elevation(elev)
        for k in NRM:
            ctx.upload_layer(k, want[k])
        ctx.run_filter("step")
        ctx.run_filter("roughness")
        ctx.sync()
        got = {k: ctx.download(k) for k in ("traversability_step", "traversability_roughness")}
        ctx.run_filter("normals")
        ctx.sync()
        got.update({k: ctx.download(k) for k in NRM})
    assert same_bits(got["traversability_step"], want["traversability_step"])
    assert_layers_match(got, want, layers=("traversability_roughness",), ctx="roughness plugin")
    wn = want_of(oracle, oracle.default_params(**radii(res, 33.5, 33.5, 40.3, 38.1)), elev, rows, cols, res)
    g, w = orient_horizontal_normals(got, wn["surface_normal_z"]), orient_horizontal_normals(wn, wn["surface_normal_z"])
    assert_layers_match(g, w, layers=NRM, ctx="normals plugin")


def test_roughness_plugin_without_points(capi, oracle):
    """RoughnessFilter with uploaded normals where the disc holds no valid elevation (0 points: score 1): option 2 against
    the generic kernel, bit for bit."""
    rows, cols, res = 130, 120, 0.01
    elev = terrain(rows, cols, seed=7550).reshape(cols, rows)
    elev[40:60, 30:55] = np.nan
    elev = elev.reshape(-1)
    op = oracle.default_params(**radii(res, 3.3, 3.3, 3.3, 3.3))
    nz = np.full(rows * cols, 0.9, np.float32)
    nx = np.full(rows * cols, np.sqrt(0.19), np.float32)
    out = []
    for option, flags in ((2, 0), (0, capi.RUN_GENERIC_KERNELS)):
        with capi.Context(0) as ctx:
            ctx.set_option(capi.OPT_FILTER_ANY_RADIUS, option)
            ctx.set_params(to_te_params(capi, op))
            ctx.set_geometry(rows, cols, 1, res)
            ctx.upload_elevation(elev)
            ctx.upload_layer("surface_normal_x", nx)
            ctx.upload_layer("surface_normal_y", np.zeros_like(nx))
            ctx.upload_layer("surface_normal_z", nz)
            ctx.run_filter("roughness", flags)
            ctx.sync()
            out.append(ctx.download("traversability_roughness"))
    assert (out[0] == 1.0).sum() > 100
    assert same_bits(out[0], out[1])


def test_precision_far_from_zero(capi, oracle, threads):
    """A plane of slope about 1 rad with 1 mm noise at +1000 m, 48-cell discs; and planes whose slope is the critical one."""
    rows, cols, res = 200, 180, 0.01
    rng = np.random.default_rng(7600)
    j, i = np.mgrid[0:cols, 0:rows]
    tilted = (1000.0 + np.tan(1.0) * res * i + rng.normal(0.0, 1e-3, (cols, rows))).astype(np.float32).reshape(-1)
    op = oracle.default_params(**radii(res, 48.2, 48.2, 5.2, 5.2), rough_critical=0.002)
    check(run(capi, op, tilted, rows, cols, res), want_of(oracle, op, tilted, rows, cols, res), "tilted plane at +1000 m")
    crit = 0.6
    plane = (np.tan(crit) * res * np.where(j < cols // 2, i, -i) + rng.normal(0.0, 1e-3, (cols, rows))).astype(np.float32).reshape(-1)
    op = oracle.default_params(**radii(res, 40.3, 40.3, 5.2, 5.2), slope_critical=crit, rough_critical=1e-3)
    want = want_of(oracle, op, plane, rows, cols, res)
    assert (np.abs(want["traversability_slope"]) < 2e-2).sum() > 100
    check(run(capi, op, plane, rows, cols, res), want, "planes at the critical slope")


def test_batch_region_graph(capi, oracle, threads):
    rows, cols, res, batch = 192, 160, 0.01, 3
    elevs = [terrain(rows, cols, seed=7700 + b, block=(b == 1)) for b in range(batch)]
    op = oracle.default_params(**radii(res, 40.3, 36.1, 34.2, 40.3))
    p = to_te_params(capi, op)
    layers = OUT_LAYERS + NRM
    n = rows * cols
    with capi.Context(0) as ctx:
        ctx.set_option(capi.OPT_FILTER_ANY_RADIUS, 1)
        ctx.set_params(p)
        ctx.set_geometry(rows, cols, batch, res)
        ctx.upload_elevation(np.concatenate(elevs))
        ctx.run_chain(capi.RUN_FOOTPRINT | capi.RUN_KEEP_NORMALS)
        ctx.sync()
        whole = {k: np.asarray(ctx.download(k, 0, batch)).reshape(-1) for k in layers + ("traversability_footprint",)}
        for b in range(batch):
            check({k: whole[k][b * n:(b + 1) * n] for k in layers}, want_of(oracle, op, elevs[b], rows, cols, res), f"map {b}")
        # a dirty tile, with and without the footprint pass behind it: the same cells as the whole-map run
        for flags in (capi.RUN_FOOTPRINT, 0):
            ctx.run_chain_region(1, 50, 40, 30, 20, flags | capi.RUN_KEEP_NORMALS)
            ctx.sync()
            for k in layers:
                assert same_bits(np.asarray(ctx.download(k, 0, batch)).reshape(-1), whole[k]), (flags, k)
            if flags:
                fp = np.asarray(ctx.download("traversability_footprint", 0, batch)).reshape(-1)
                assert_layers_match({"f": fp}, {"f": whole["traversability_footprint"]}, layers=("f",), tol=1e-6, ctx="region footprint")
    # graph replay, twice
    outs = []
    with capi.Context(0) as ctx:
        ctx.set_option(capi.OPT_FILTER_ANY_RADIUS, 1)
        ctx.set_option(capi.OPT_GRAPH_REPLAY, 1)
        ctx.set_params(p)
        ctx.set_geometry(rows, cols, batch, res)
        ctx.upload_elevation(np.concatenate(elevs))
        for _ in range(2):
            ctx.run_chain(capi.RUN_KEEP_NORMALS)
            ctx.sync()
            outs.append({k: np.asarray(ctx.download(k, 0, batch)).reshape(-1) for k in layers})
    for k in layers:
        assert same_bits(outs[0][k], whole[k]) and same_bits(outs[1][k], whole[k]), k


@pytest.mark.parametrize("cells", [1.0, 3.2, 9.4, 9.0, 20.3], ids=["1-cell tie", "3", "9", "9 tie", "20"])
def test_forced_route_small_discs(capi, oracle, threads, cells):
    """Option 2 where the shape kernels also run: the oracle, the default route and the generic kernels within 1e-5; step
    layers bit for bit."""
    rows = cols = 1024
    res = 0.01
    elev = terrain(rows, cols, seed=7800 + int(cells * 10), holes=0.002, boxes=60, block=True)
    op = oracle.default_params(**radii(res, cells, cells, cells, cells))
    got = run(capi, op, elev, rows, cols, res, option=2)
    ref = run(capi, op, elev, rows, cols, res, option=0)
    generic = run(capi, op, elev, rows, cols, res, option=0, flags=capi.RUN_GENERIC_KERNELS)
    # (normals to 1e-4: on a million cells a disc whose two smallest eigenvalues nearly coincide turns its eigenvector by
    # 2e-5 between the generic arithmetic and the oracle's -- the scores stay within 1e-5)
    check(got, want_of(oracle, op, elev, rows, cols, res), f"forced, {cells} cells", normals_tol=1e-4)
    assert_layers_match(got, ref, ctx=f"forced vs default, {cells} cells")
    assert same_bits(got["traversability_step"], ref["traversability_step"])
    assert_layers_match(got, generic, ctx=f"forced vs generic, {cells} cells")
    assert same_bits(got["traversability_step"], generic["traversability_step"])


# TE_FILTER_ANY_CASES="first:count" widens the sweep (default: 24 cases)
_first, _count = (int(v) for v in os.environ.get("TE_FILTER_ANY_CASES", "0:24").split(":"))


@pytest.mark.parametrize("case", range(_first, _first + _count))
def test_random_sweep(capi, oracle, threads, case):
    rng = np.random.default_rng(80000 + case)
    rows, cols = (int(v) for v in rng.integers(64, 241, 2))
    res = float(rng.choice([0.01, 0.02, 0.05]))
    r = [float(v) for v in rng.uniform(20.0, 80.0, 4)]
    if rng.random() < 0.25:
        r[int(rng.integers(0, 4))] = float(rng.integers(20, 81))  # a whole-cell (tie) radius
    op = oracle.default_params(**radii(res, *r), normals_axis=int(rng.choice([2, 2, 2, 0, 1])))
    elev = terrain(rows, cols, seed=81000 + case, holes=float(rng.choice([0.0, 0.003, 0.03])), block=bool(rng.random() < 0.3))
    pos = tuple(float(v) for v in rng.uniform(-2.0, 2.0, 2))
    check(run(capi, op, elev, rows, cols, res, pos), want_of(oracle, op, elev, rows, cols, res, pos), f"case {case}: {rows}x{cols} {res} {r}")


def test_rank_rule_refused_with_a_large_normals_disc(capi, oracle):
    """TE_OPT_NORMALS_RANK_RULE with a normals disc of the route of any radius: refused (TE_ERR_UNSUPPORTED), not guessed."""
    rows, cols, res = 120, 100, 0.01
    elev = terrain(rows, cols, seed=7950)
    with capi.Context(0) as ctx:
        ctx.set_option(capi.OPT_FILTER_ANY_RADIUS, 1)
        ctx.set_option(capi.OPT_NORMALS_RANK_RULE, 1)
        ctx.set_params(to_te_params(capi, oracle.default_params(**radii(res, 40.3, 40.3, 3.3, 3.3))))
        ctx.set_geometry(rows, cols, 1, res)
        ctx.upload_elevation(elev)
        for call in (lambda: ctx.run_chain(0), lambda: ctx.run_filter("normals")):
            with pytest.raises(capi.TeError) as e:
                call()
            assert e.value.code == ERR_UNSUPPORTED
        ctx.set_option(capi.OPT_GRAPH_REPLAY, 1)  # (refused before a capture, not inside one)
        with pytest.raises(capi.TeError):
            ctx.run_chain(0)
        ctx.set_option(capi.OPT_NORMALS_RANK_RULE, 0)
        ctx.run_chain(capi.RUN_KEEP_NORMALS)
        ctx.sync()
        got = {k: ctx.download(k) for k in OUT_LAYERS + NRM}
    check(got, want_of(oracle, oracle.default_params(**radii(res, 40.3, 40.3, 3.3, 3.3)), elev, rows, cols, res), "rank rule off again")


def test_tables_beyond_lds(capi, oracle, threads):
    """1000-cell discs on a 2100-row map: the step tables and the normals prefix sums outgrow 64 KiB of LDS and the plain
    gathers (k_fa_step_exact, k_fa_exact) serve; the same results."""
    rows, cols, res = 2100, 24, 0.005
    elev = terrain(rows, cols, seed=7960, boxes=8)
    op = oracle.default_params(**radii(res, 1000.3, 1000.3, 1000.3, 990.2))
    check(run(capi, op, elev, rows, cols, res), want_of(oracle, op, elev, rows, cols, res), "1000 cells on 2100 x 24")
