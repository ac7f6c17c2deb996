"""The context's validity state as the entry points show it (te_ctx_state.h; its model: tests/test_ctx_state.py).  Short call
sequences on one context, each compared with a fresh context that does the plain thing -- upload, te_run_chain with the
footprint flag -- bit for bit on every output layer, and every refusal by its code.  Maps of 80 x 72: 80 rows still take the
wavefront-wide routes, and 72 columns would show a transposed index."""
import numpy as np
import pytest

from tests.helpers import OUT_LAYERS

pytestmark = pytest.mark.gpu

ROWS, COLS, RES = 80, 72, 0.05
LAYERS = list(OUT_LAYERS) + ["traversability_footprint"]
ERR_NOT_READY = -3


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import capi
    capi.load()
    assert capi.device_count() >= 1
    return capi


@pytest.fixture(scope="module")
def elev():
    from traversability_estimation_amd import synth
    e = synth.with_steps(synth.perlin_elevation(ROWS, COLS, seed=41, amplitude=0.12), 6, seed=48)
    e = synth.with_holes(e, 0.004, seed=42)
    e[COLS // 2:COLS // 2 + 4, 20:45] = np.nan
    return e


def _params(capi, **over):
    from traversability_estimation_amd import synth
    r = synth.benchmark_radius(4, RES)
    kw = dict(normals_radius=r, rough_radius=r, step_radius1=r, step_radius2=r, fp_radius=synth.benchmark_radius(4, RES),
              fp_offset=synth.benchmark_radius(2, RES))
    kw.update(over)
    return capi.default_params(**kw)


def _ready(capi, ctx, elev, p):
    ctx.set_params(p)
    ctx.set_geometry(ROWS, COLS, 1, RES)
    ctx.upload_elevation(elev)


def _plain(capi, elev, p):
    """The plain thing on a fresh context: upload, chain with the footprint flag, download."""
    with capi.Context(0) as ctx:
        _ready(capi, ctx, elev, p)
        ctx.run_chain(capi.RUN_FOOTPRINT)
        ctx.sync()
        return {k: ctx.download(k) for k in LAYERS}


@pytest.fixture(scope="module")
def plain(capi, elev):
    return _plain(capi, elev, _params(capi))


def _same(got, want):
    for k in LAYERS:
        a, b = got[k], want[k]
        both_nan = np.isnan(a) & np.isnan(b)
        assert np.array_equal(a.view(np.uint32)[~both_nan], b.view(np.uint32)[~both_nan]), k


def _refused(capi, call):
    with pytest.raises(capi.TeError) as e:
        call()
    assert e.value.code == ERR_NOT_READY


def test_replay_and_direct_launches_leave_the_same_layers_and_state(capi, elev, plain):
    """A replayed whole-map launch leaves what the direct launches leave: the layers, and a context that accepts a region
    run with the footprint flag (chain_done, footprint_done)."""
    with capi.Context(0) as ctx:
        _ready(capi, ctx, elev, _params(capi))
        for mode in (1, 2):  # always replayed (capture, then a replay), never
            ctx.set_option(capi.OPT_GRAPH_REPLAY, mode)
            for _ in range(2):
                ctx.run_chain(capi.RUN_FOOTPRINT)
            ctx.sync()
            _same({k: ctx.download(k) for k in LAYERS}, plain)
            ctx.run_chain_region(0, 8, 16, 24, 16, capi.RUN_FOOTPRINT)  # (accepted; the next whole-map run rewrites every cell)
            ctx.sync()


def test_a_new_footprint_radius_keeps_the_chain(capi, elev):
    from traversability_estimation_amd import synth
    wider = _params(capi, fp_radius=synth.benchmark_radius(6, RES))
    with capi.Context(0) as ctx:
        _ready(capi, ctx, elev, _params(capi))
        ctx.run_chain(capi.RUN_FOOTPRINT)
        ctx.set_params(wider)
        ctx.run_footprint()  # (no new chain)
        ctx.sync()
        got = {k: ctx.download(k) for k in LAYERS}
    _same(got, _plain(capi, elev, wider))


def test_a_new_filter_parameter_withdraws_the_chain(capi, elev):
    with capi.Context(0) as ctx:
        _ready(capi, ctx, elev, _params(capi))
        ctx.run_chain(capi.RUN_FOOTPRINT)
        ctx.set_params(_params(capi, step_critical=0.2))
        _refused(capi, ctx.run_footprint)


def test_an_uploaded_score_layer_rebuilds_the_mask_of_the_path_check(capi, elev, plain):
    r = 0.2
    paths = [np.stack([np.linspace(-1.5, 1.5, 12), np.full(12, y)], axis=1) for y in (-1.0, -0.3, 0.0, 0.4, 1.1)]
    slope = plain["traversability_slope"].copy().reshape(COLS, ROWS)
    slope[20:52, 24:56] = 0.0  # a block the slope filter would call untraversable
    with capi.Context(0) as ctx:
        _ready(capi, ctx, elev, _params(capi))
        ctx.run_chain(capi.RUN_FOOTPRINT)
        before = ctx.check_footprint_paths_radius(paths, r)
        ctx.upload_layer("traversability_slope", slope)
        got = ctx.check_footprint_paths_radius(paths, r)
    with capi.Context(0) as ctx:  # a fresh context given the same four layers
        _ready(capi, ctx, elev, _params(capi))
        ctx.run_chain(0)
        ctx.upload_layer("traversability_slope", slope)
        for k in ("traversability_step", "traversability_roughness", "traversability"):
            ctx.upload_layer(k, plain[k])
        want = ctx.check_footprint_paths_radius(paths, r)
    for g, w in zip(got, want):
        assert np.array_equal(g, w, equal_nan=g.dtype.kind == "f")
    assert not np.array_equal(before[0], got[0])  # (the block is seen: the mask was built again)


def test_face_flags_are_withdrawn_for_good_once_the_elevation_pointer_is_out(capi, elev):
    with capi.Context(0) as ctx:
        _ready(capi, ctx, elev, _params(capi))
        assert ctx.download_face_flags().shape == (1, COLS // 4, 2)
        ctx.device_ptr("elevation")
        _refused(capi, ctx.download_face_flags)
        ctx.upload_elevation(elev)
        _refused(capi, ctx.download_face_flags)


def test_a_single_filter_withdraws_the_chain(capi, elev):
    with capi.Context(0) as ctx:
        _ready(capi, ctx, elev, _params(capi))
        ctx.run_chain(capi.RUN_FOOTPRINT)
        ctx.run_chain_region(0, 8, 16, 24, 16, 0)
        ctx.run_filter("slope")
        _refused(capi, lambda: ctx.run_chain_region(0, 8, 16, 24, 16, 0))
