"""What te_run_median_fill, te_run_radius_filter and te_run_window_expression have in common (the contract: csrc/te_layer_call.h):
the binding of a call to its layers, the copy an in-place call reads, the block counts, and the event-timed loop of their
te_time_*_samples, which no other test runs on the device.
Every comparison is between two runs on the device and bit for bit; the values themselves are checked against the numpy
references in test_gpu_median_fill.py, test_gpu_radius_filter.py and test_gpu_window_expression.py."""
import numpy as np
import pytest

from tests import median_fill_cases as M
from tests import radius_filter_cases as K

pytestmark = pytest.mark.gpu

ROWS, COLS, BATCH = 70, 37, 2
OUT = "traversability_roughness"
FILTERS = ("median", "radius", "window")


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    return capi


@pytest.fixture(scope="module")
def maps():
    flat = np.ascontiguousarray(np.stack([m.T for m in K.holey_maps(ROWS, COLS, BATCH, 41, ["speckle_5"])]), np.float32).reshape(-1)
    flat.setflags(write=False)
    return flat


class Filter:
    """One of the three filters behind the same four calls; `src` and `dst` are layer names (`dst` also an id)."""

    def __init__(self, capi, name):
        self.capi, self.name = capi, name
        self.median = capi.default_median_fill_params(fill_hole_radius=M.radius_for(1), num_erode_dilation_iterations=1)
        self.window = capi.window_expr_params(window_size=3)
        self.radius = K.radius_of(1.5)

    def run(self, ctx, src="elevation", dst=OUT, **maps):
        if self.name == "median":
            ctx.run_median_fill(self.median, src, dst, **maps)
        elif self.name == "radius":
            ctx.run_radius_filter(K.MEAN, self.radius, src, dst, **maps)
        else:
            ctx.run_window_expression(f"mean({src})", self.window, src, dst, **maps)

    def timed(self, ctx, src="elevation", dst=OUT, warmup=1, iters=2, floor=False):
        if self.name == "median":
            return ctx.time_median_fill_samples(None if floor else self.median, src, dst, warmup, iters)
        if self.name == "radius":
            return ctx.time_radius_filter_samples(0 if floor else K.MEAN, self.radius, src, dst, warmup, iters)
        return ctx.time_window_expression_samples(None if floor else f"mean({src})", self.window, src, dst, warmup, iters)

    def state(self, ctx):
        """What a run leaves beside its layer: the fill masks of both maps, or the two block counts."""
        if self.name == "median":
            return tuple(ctx.download_fill_mask(m).tobytes() for m in range(BATCH))
        return ctx.radius_filter_stats() if self.name == "radius" else ctx.window_expression_stats()


def context(capi, rows=ROWS, cols=COLS, elevation=None):
    ctx = capi.Context(0)
    ctx.set_params(capi.default_params())
    ctx.set_geometry(rows, cols, BATCH, K.RES)
    if elevation is not None:
        ctx.upload_elevation(elevation)
    return ctx


def bits(ctx, layer):
    return ctx.download(layer).view(np.uint32)


def refused(capi, code, call, *args, **kw):
    with pytest.raises(capi.TeError) as e:
        call(*args, **kw)
    assert e.value.code == code, str(e.value)


@pytest.mark.parametrize("name", FILTERS)
def test_timed_run_equals_plain_run(capi, maps, name):
    f = Filter(capi, name)
    with context(capi, elevation=maps) as a, context(capi, elevation=maps) as b:
        ms = f.timed(a)
        f.run(b)
        assert ms.shape == (2,) and np.all(np.isfinite(ms)) and np.all(ms > 0.0), ms
        assert np.array_equal(bits(a, OUT), bits(b, OUT))
        assert f.state(a) == f.state(b)
        assert np.array_equal(bits(a, "elevation"), maps.view(np.uint32))


@pytest.mark.parametrize("name", FILTERS)
def test_the_floor_is_a_copy(capi, maps, name):
    f = Filter(capi, name)
    with context(capi, elevation=maps) as ctx:
        ms = f.timed(ctx, floor=True)
        assert ms.shape == (2,) and np.all(np.isfinite(ms)) and np.all(ms > 0.0), ms
        assert np.array_equal(bits(ctx, OUT), maps.view(np.uint32))
        refused(capi, capi.TE_ERR_NOT_READY, f.state, ctx)  # a copy leaves neither counts nor a mask


@pytest.mark.parametrize("name", FILTERS)
def test_timed_refusals(capi, name):
    f = Filter(capi, name)
    with capi.Context(0) as ctx:
        refused(capi, capi.TE_ERR_NOT_READY, f.timed, ctx)  # no geometry
    with context(capi, 16, 9, np.zeros(BATCH * 16 * 9, np.float32)) as ctx:
        refused(capi, capi.TE_ERR_INVALID_ARG, f.timed, ctx, "elevation", "elevation")
        refused(capi, capi.TE_ERR_INVALID_ARG, f.timed, ctx, iters=0)


def test_three_filters_in_place_equal_the_chain_out_of_place(capi, maps):
    fs = [Filter(capi, name) for name in ("radius", "window", "median")]
    chain = ("elevation", OUT, "traversability_slope", "traversability_step")
    with context(capi, elevation=maps) as a, context(capi, elevation=maps) as b:
        for k, f in enumerate(fs):
            f.run(a, "elevation", "elevation")
            f.run(b, chain[k], chain[k + 1])
        assert np.array_equal(bits(a, "elevation"), bits(b, chain[-1]))
        assert not np.array_equal(bits(a, "elevation"), maps.view(np.uint32))


@pytest.mark.parametrize("name", FILTERS)
def test_a_refused_call_changes_nothing(capi, name):
    f = Filter(capi, name)
    elevation = np.ascontiguousarray(np.stack([m.T for m in K.holey_maps(16, 9, BATCH, 43, ["speckle_5"])]), np.float32).reshape(-1)
    with context(capi, 16, 9, elevation) as ctx:
        f.run(ctx)
        layer, state = bits(ctx, OUT), f.state(ctx)
        refused(capi, capi.TE_ERR_INVALID_ARG, f.run, ctx, map0=1, nmaps=2)
        refused(capi, capi.TE_ERR_INVALID_ARG, f.run, ctx, dst=12)
        assert np.array_equal(bits(ctx, OUT), layer)
        assert f.state(ctx) == state


def pointwise_call(name):
    """te_copy_layer, te_run_threshold or te_run_layer_expression reading `src`, writing `dst`; `maps` where the call takes them."""
    def call(ctx, src="elevation", dst=OUT, **maps):
        if name == "copy":
            ctx.copy_layer(src, dst, **maps)
        elif name == "threshold":
            ctx.run_threshold(dst, "lower", 0.0, 1.0, **maps)
        else:
            assert not maps
            ctx.run_layer_expression(f"2 * {src}" if isinstance(src, str) else "2 * elevation", dst)
    return call


@pytest.mark.parametrize("shape", [(ROWS, COLS), (16, 9)])
@pytest.mark.parametrize("name", ("copy", "threshold", "layer_expression"))
def test_a_refused_pointwise_call_changes_nothing(capi, name, shape):
    """A bad map range and a user id that was never added: the layers of the call, the block counts of the radius filter before
    it and the user layers' absence are afterwards what they were."""
    rows, cols = shape
    call = pointwise_call(name)
    unadded = len(capi.LAYERS) + 3
    elevation = np.ascontiguousarray(np.stack([m.T for m in K.holey_maps(rows, cols, BATCH, 43, ["speckle_5"])]), np.float32).reshape(-1)
    with context(capi, rows, cols, elevation) as ctx:
        Filter(capi, "radius").run(ctx)
        call(ctx)
        layers = {k: bits(ctx, k) for k in ("elevation", OUT)}
        state = ctx.radius_filter_stats()
        if name == "layer_expression":  # (the whole-map call takes no maps: its region form names one)
            refused(capi, capi.TE_ERR_INVALID_ARG, ctx.run_layer_expression_region, "2 * elevation", OUT, BATCH, 0, 0, 4, 4)
            refused(capi, capi.TE_ERR_INVALID_ARG, ctx.run_layer_expression_region, "2 * elevation", OUT, -1, 0, 0, 4, 4)
        else:
            refused(capi, capi.TE_ERR_INVALID_ARG, call, ctx, map0=1, nmaps=2)
            refused(capi, capi.TE_ERR_INVALID_ARG, call, ctx, map0=BATCH, nmaps=1)
        refused(capi, capi.TE_ERR_INVALID_ARG, call, ctx, dst=unadded)
        if name == "copy":
            refused(capi, capi.TE_ERR_INVALID_ARG, call, ctx, src=unadded)
        for k, v in layers.items():
            assert np.array_equal(bits(ctx, k), v), k
        assert ctx.radius_filter_stats() == state
        refused(capi, capi.TE_ERR_INVALID_ARG, ctx.download, unadded)
