"""NormalVectorsFilter's raster method on the device (TE_OPT_NORMALS_ALGORITHM = 1, k_normals_raster): the normals bit for bit
against the numpy statement of the contract (tests/ref_py/raster_normals_ref.py, NaN patterns included), the chain behind them
against the oracle's single filters fed those normals, within the suite's 1e-5 (tests/helpers.py).

Shapes: 3 x 3 (one interior cell), 2 x 7 (none), 67 x 45 and 65 x 33 (no multiple of the 64 x 4 block; one and two blocks along the
rows), 128 x 64 (whole blocks), 131 x 70 with batch 3.  Inputs: smooth relief; 10 % scattered NaN plus a NaN block plus a few
+-inf; all NaN.  A single-map shape runs the three inputs one after the other on one context, the batch holds one each."""
import functools
import os

import numpy as np
import pytest

from tests.helpers import TOL, compare_layer, to_te_params
from tests.ref_py import raster_normals_ref as R

pytestmark = pytest.mark.gpu

RES = 0.03
POS = (0.4, -1.1)
SHAPES = [(3, 3, 1), (2, 7, 1), (67, 45, 1), (65, 33, 1), (128, 64, 1), (131, 70, 3)]
INPUTS = ("smooth", "holes", "all_nan")
NRM = ("surface_normal_x", "surface_normal_y", "surface_normal_z")
SCORES = ("traversability_slope", "traversability_step", "traversability_roughness", "traversability")
ROUGH_CELLS = (1.5, 5.0 * (1.0 + 1e-6), 9.0)  # generic-sized, the sliding kernel's tie-free radius, a tie radius


def _ids(shapes=SHAPES):
    return [f"{r}x{c}x{b}" for r, c, b in shapes]


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no MI355X visible"
    return capi


@pytest.fixture(scope="module", autouse=True)
def threads(oracle):
    oracle.set_threads(min(os.cpu_count() or 1, 16))
    yield
    oracle.set_threads(1)


def bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def elevation(rows, cols, kind):
    """One map, flat column-major float32 (read-only: shared between the tests)."""
    rng = np.random.default_rng(rows * 1000 + cols)
    i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    z = (0.35 * np.sin(i * 0.21) * np.cos(j * 0.17) + 0.02 * i - 0.015 * j + 0.004 * rng.normal(size=(rows, cols))).astype(np.float32)
    if kind == "holes":
        z[rng.random((rows, cols)) < 0.10] = np.nan
        z[rows // 3:rows // 3 + max(1, rows // 5), cols // 4:cols // 4 + max(1, cols // 4)] = np.nan
        for k in range(min(6, rows * cols // 4)):
            z[rng.integers(rows), rng.integers(cols)] = np.inf if k % 2 else -np.inf
    elif kind == "all_nan":
        z[:] = np.nan
    flat = R.as_flat(z)
    flat.setflags(write=False)
    return flat


def maps_of(rows, cols, batch):
    """The uploads of a shape: lists of `batch` maps."""
    if batch == 3:
        return [[elevation(rows, cols, k) for k in INPUTS]]
    return [[elevation(rows, cols, k)] for k in INPUTS]


@functools.lru_cache(maxsize=None)
def ref_normals(rows, cols, kind, axis):
    out = R.raster_normals_flat(elevation(rows, cols, kind), rows, cols, RES, axis)
    for v in out:
        v.setflags(write=False)
    return out


def kind_of(rows, cols, e):
    return next(k for k in INPUTS if elevation(rows, cols, k) is e)


_ORACLE = {}


def ref_chain(oracle, rows, cols, kind, rough_cells, axis=2):
    """The reference's chain on the raster normals of the numpy reference: computed once per case."""
    key = (rows, cols, kind, rough_cells, axis)
    if key not in _ORACLE:
        op = params(oracle, rough_cells, axis)
        g = oracle.geom(rows, cols, RES, POS)
        e = elevation(rows, cols, kind)
        nx, ny, nz = ref_normals(rows, cols, kind, axis)
        out = dict(zip(NRM, (nx, ny, nz)))
        out["traversability_slope"] = oracle.slope(g, nz, op.slope_critical)
        out["traversability_step"] = oracle.step(g, e, op.step_critical, op.step_radius1, op.step_radius2, op.step_ncrit)
        out["traversability_roughness"] = oracle.roughness(g, e, nx, ny, nz, op.rough_critical, op.rough_radius)
        out["traversability"] = oracle.combine(out["traversability_slope"], out["traversability_step"], out["traversability_roughness"], op.w_scale,
                                               op.w_slope, op.w_step, op.w_rough)
        _ORACLE[key] = out
    return _ORACLE[key]


def params(oracle, rough_cells=5.0 * (1.0 + 1e-6), axis=2, normals_cells=2.0):
    return oracle.default_params(normals_radius=normals_cells * RES, normals_axis=axis, rough_radius=rough_cells * RES, rough_critical=0.08,
                                 step_radius1=2.0 * RES * (1.0 + 1e-6), step_radius2=1.5 * RES)


def context(capi, oracle, rows, cols, batch, raster=1, any_radius=0, graph=None, **over):
    ctx = capi.Context(0)
    if any_radius:
        ctx.set_option(capi.OPT_FILTER_ANY_RADIUS, any_radius)
    if graph is not None:
        ctx.set_option(capi.OPT_GRAPH_REPLAY, graph)
    ctx.set_option(capi.OPT_NORMALS_ALGORITHM, raster)
    ctx.set_params(to_te_params(capi, params(oracle, **over)))
    ctx.set_geometry(rows, cols, batch, RES, POS)
    return ctx


def layers(ctx, names, b):
    return {k: ctx.download(k, b, 1) for k in names}


def check_scores(got, want, what):
    for k in SCORES:
        n_bad, worst, nan_bad = compare_layer(k, got[k], want[k], TOL)
        print(f"{what}: {k} max|d| = {worst:.3g}, NaN-pattern mismatches {nan_bad}")
        assert nan_bad == 0 and n_bad == 0, (what, k, n_bad, worst, nan_bad)


# ---- (f) TE_FILTER_NORMALS --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,cols,batch", SHAPES, ids=_ids())
def test_f_normals_filter_is_the_reference_bit_for_bit(capi, oracle, rows, cols, batch):
    """The three layers of te_run_filter(normals) under raster, every cell, every positive axis; the other layers stay as they
    were (NaN since te_set_geometry) and the elevation is not touched."""
    for axis in (2, 0, 1):
        with context(capi, oracle, rows, cols, batch, axis=axis) as ctx:
            for maps in maps_of(rows, cols, batch):
                ctx.upload_elevation(np.concatenate(maps))
                ctx.run_filter("normals")
                ctx.sync()
                for b, e in enumerate(maps):
                    kind = kind_of(rows, cols, e)
                    got = layers(ctx, NRM, b)
                    for name, want in zip(NRM, ref_normals(rows, cols, kind, axis)):
                        bad = np.flatnonzero(bits(got[name]) != bits(want))
                        assert bad.size == 0, (axis, kind, name, [(int(o % rows), int(o // rows), float(got[name][o]), float(want[o])) for o in bad[:6]])
                    if kind == "smooth" and min(rows, cols) >= 3:
                        assert np.isfinite(got[NRM[2]]).sum() == (rows - 2) * (cols - 2)
                    for name in SCORES:
                        assert np.isnan(ctx.download(name, b, 1)).all(), name
                assert same_bits(ctx.download("elevation"), np.concatenate(maps))


# ---- (g) the chain, normals kept --------------------------------------------------------------------------------------------------

def run_g(capi, oracle, rows, cols, batch, cells, any_radius=0, flags=0, keep=True):
    """te_run_chain under raster on every input of the shape: {(kind): layers}."""
    out = {}
    with context(capi, oracle, rows, cols, batch, any_radius=any_radius, rough_cells=cells) as ctx:
        for maps in maps_of(rows, cols, batch):
            ctx.upload_elevation(np.concatenate(maps))
            ctx.run_chain(flags | (capi.RUN_KEEP_NORMALS if keep else 0))
            ctx.sync()
            for b, e in enumerate(maps):
                out[kind_of(rows, cols, e)] = layers(ctx, SCORES + (NRM if keep else ()), b)
    return out


@pytest.mark.parametrize("cells", ROUGH_CELLS, ids=["r1.5", "r5tf", "r9tie"])
@pytest.mark.parametrize("rows,cols,batch", SHAPES, ids=_ids())
def test_g_chain_with_kept_normals(capi, oracle, rows, cols, batch, cells):
    got = run_g(capi, oracle, rows, cols, batch, cells)
    for kind, layer in got.items():
        want = ref_chain(oracle, rows, cols, kind, cells)
        for name in NRM:
            assert same_bits(layer[name], want[name]), (kind, name)
        check_scores(layer, want, f"{rows}x{cols}x{batch} {kind} r={cells:g}")
        if kind == "all_nan":
            assert all(np.isnan(layer[k]).all() for k in SCORES)


@pytest.mark.parametrize("rows,cols,batch", [(67, 45, 1), (131, 70, 3)], ids=_ids([(67, 45, 1), (131, 70, 3)]))
def test_g_chain_on_the_route_of_any_radius(capi, oracle, rows, cols, batch):
    """TE_OPT_FILTER_ANY_RADIUS = 2: every filter disc on te_filter_any.hip, the roughness on given normals among them."""
    cells = ROUGH_CELLS[1]
    for kind, layer in run_g(capi, oracle, rows, cols, batch, cells, any_radius=2).items():
        want = ref_chain(oracle, rows, cols, kind, cells)
        for name in NRM:
            assert same_bits(layer[name], want[name]), (kind, name)
        check_scores(layer, want, f"any radius {rows}x{cols}x{batch} {kind}")


# ---- (h) without TE_RUN_KEEP_NORMALS ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,cols,batch", [(65, 33, 1), (131, 70, 3)], ids=_ids([(65, 33, 1), (131, 70, 3)]))
def test_h_scores_without_kept_normals(capi, oracle, rows, cols, batch):
    """The same score bits as (g); the normal layers count as absent afterwards, as they do under area: nothing in the library
    refuses te_download_layer of them (it never has), the calls that ask whether a layer exists do -- te_run_expression."""
    cells = ROUGH_CELLS[1]
    kept = run_g(capi, oracle, rows, cols, batch, cells)
    plain = run_g(capi, oracle, rows, cols, batch, cells, keep=False)
    for kind in kept:
        for k in SCORES:
            assert same_bits(kept[kind][k], plain[kind][k]), (kind, k)
    for raster in (1, 0):
        with context(capi, oracle, rows, cols, batch, raster=raster, rough_cells=cells) as ctx:
            ctx.upload_elevation(np.concatenate(maps_of(rows, cols, batch)[0]))
            ctx.run_chain(capi.RUN_KEEP_NORMALS)
            ctx.run_expression("surface_normal_z")
            ctx.run_chain(0)
            with pytest.raises(capi.TeError) as err:
                ctx.run_expression("surface_normal_z")
            assert err.value.code == capi.TE_ERR_NOT_READY and "surface_normal_z" in str(err.value), raster


# ---- (i) normals_radius plays no part ---------------------------------------------------------------------------------------------

def test_i_the_normals_radius_changes_nothing(capi, oracle):
    rows, cols, batch = 131, 70, 3
    got = []
    for normals_cells in (2.0, 7.0 * (1.0 + 1e-6)):
        with context(capi, oracle, rows, cols, batch, normals_cells=normals_cells) as ctx:
            ctx.upload_elevation(np.concatenate(maps_of(rows, cols, batch)[0]))
            ctx.run_chain(capi.RUN_KEEP_NORMALS)
            ctx.sync()
            got.append({k: ctx.download(k) for k in SCORES + NRM})
    for k in SCORES + NRM:
        assert same_bits(got[0][k], got[1][k]), k
    assert np.isfinite(got[0]["traversability"]).any()


# ---- (j) the footprint pass behind the raster chain -------------------------------------------------------------------------------

@pytest.mark.parametrize("sequential", [False, True], ids=["deferred-combine", "sequential"])
def test_j_footprint_behind_the_raster_chain(capi, oracle, sequential):
    """TE_RUN_FOOTPRINT: the combine is left to the mask kernel (or, sequential, done by k_combine); the footprint layer is the
    oracle's on the device's own raster layers."""
    rows, cols, batch = 131, 70, 3
    op = params(oracle)
    g = oracle.geom(rows, cols, RES, POS)
    maps = maps_of(rows, cols, batch)[0]
    flags = capi.RUN_FOOTPRINT | capi.RUN_KEEP_NORMALS | (capi.RUN_SEQUENTIAL if sequential else 0)
    with context(capi, oracle, rows, cols, batch) as ctx:
        ctx.upload_elevation(np.concatenate(maps))
        ctx.run_chain(flags)
        ctx.sync()
        for b, e in enumerate(maps):
            kind = kind_of(rows, cols, e)
            got = layers(ctx, SCORES + NRM + ("traversability_footprint",), b)
            want = ref_chain(oracle, rows, cols, kind, 5.0 * (1.0 + 1e-6))
            for name in NRM:
                assert same_bits(got[name], want[name]), (kind, name)
            check_scores(got, want, f"footprint run, {kind}")
            fp = oracle.footprint(g, op, e, got)
            n_bad, worst, nan_bad = compare_layer("traversability_footprint", got["traversability_footprint"], fp, TOL)
            print(f"footprint, {kind}: max|d| = {worst:.3g}")
            assert n_bad == 0 and nan_bad == 0, (kind, n_bad, worst, nan_bad)


# ---- (k) area -> raster -> area on one context, graph replay forced on ------------------------------------------------------------

def test_k_switching_the_algorithm_with_graph_replay(capi, oracle):
    rows, cols, batch = 131, 70, 3
    elev = np.concatenate(maps_of(rows, cols, batch)[0])
    names = SCORES + NRM

    def run(ctx):
        ctx.run_chain(capi.RUN_KEEP_NORMALS)
        ctx.run_chain(capi.RUN_KEEP_NORMALS)  # (the second launch replays the captured graph)
        ctx.sync()
        return {k: ctx.download(k) for k in names}

    fresh = {}
    for raster in (0, 1):
        with context(capi, oracle, rows, cols, batch, raster=raster, graph=1) as ctx:
            ctx.upload_elevation(elev)
            fresh[raster] = run(ctx)
    assert not same_bits(fresh[0]["surface_normal_z"], fresh[1]["surface_normal_z"])
    with context(capi, oracle, rows, cols, batch, raster=0, graph=1) as ctx:
        ctx.upload_elevation(elev)
        for raster in (0, 1, 0, 1):
            ctx.set_option(capi.OPT_NORMALS_ALGORITHM, raster)
            got = run(ctx)
            for k in names:
                assert same_bits(got[k], fresh[raster][k]), (raster, k)
        for bad in (2, -1):
            with pytest.raises(capi.TeError) as err:
                ctx.set_option(capi.OPT_NORMALS_ALGORITHM, bad)
            assert err.value.code == capi.TE_ERR_INVALID_ARG


# ---- (l) te_run_chain_region ------------------------------------------------------------------------------------------------------

def test_l_region_runs_are_refused(capi, oracle):
    rows, cols, batch = 67, 45, 1
    names = SCORES + NRM
    with context(capi, oracle, rows, cols, batch) as ctx:
        ctx.upload_elevation(elevation(rows, cols, "holes"))
        ctx.run_chain(capi.RUN_KEEP_NORMALS)
        ctx.sync()
        before = {k: ctx.download(k) for k in names}
        with pytest.raises(capi.TeError) as err:
            ctx.run_chain_region(0, 10, 10, 8, 8)
        assert err.value.code == capi.TE_ERR_UNSUPPORTED and "TE_OPT_NORMALS_ALGORITHM" in str(err.value)
        ctx.sync()
        for k in names:
            assert same_bits(ctx.download(k), before[k]), k
        ctx.set_option(capi.OPT_NORMALS_ALGORITHM, 0)  # (area: the region form is there, after a whole run)
        ctx.run_chain(0)
        ctx.run_chain_region(0, 10, 10, 8, 8)
        ctx.sync()


# ---- (m) the rank rule ------------------------------------------------------------------------------------------------------------

def test_m_the_rank_rule_changes_nothing_under_raster(capi, oracle):
    """Also with a normals disc of the route of any radius, which the rule refuses under area."""
    rows, cols, batch = 131, 70, 3
    elev = np.concatenate(maps_of(rows, cols, batch)[0])
    got = []
    for rule in (0, 1):
        with context(capi, oracle, rows, cols, batch) as ctx:
            ctx.set_option(capi.OPT_NORMALS_RANK_RULE, rule)
            ctx.upload_elevation(elev)
            ctx.run_chain(capi.RUN_KEEP_NORMALS)
            ctx.sync()
            got.append({k: ctx.download(k) for k in SCORES + NRM})
            ctx.run_filter("normals")
            ctx.sync()
            for k in NRM:
                assert same_bits(ctx.download(k), got[-1][k]), (rule, k)
    for k in SCORES + NRM:
        assert same_bits(got[0][k], got[1][k]), k
    with context(capi, oracle, rows, cols, batch, any_radius=2) as ctx:
        ctx.set_option(capi.OPT_NORMALS_RANK_RULE, 1)
        ctx.upload_elevation(elev)
        ctx.run_chain(capi.RUN_KEEP_NORMALS)
        ctx.sync()
        for k in NRM:
            assert same_bits(ctx.download(k), got[0][k]), k


def test_normals_only_writes_the_normals_and_nothing_else(capi, oracle):
    rows, cols, batch = 65, 33, 1
    with context(capi, oracle, rows, cols, batch) as ctx:
        ctx.upload_elevation(elevation(rows, cols, "holes"))
        ctx.run_chain(capi.RUN_NORMALS_ONLY)
        ctx.sync()
        for name, want in zip(NRM, ref_normals(rows, cols, "holes", 2)):
            assert same_bits(ctx.download(name), want), name
        for name in SCORES:
            assert np.isnan(ctx.download(name)).all(), name
