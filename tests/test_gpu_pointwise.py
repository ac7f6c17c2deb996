"""te_run_threshold(_region) and te_copy_layer against the numpy contract (tests/ref_py/pointwise_ref.py), and the fused call
te_run_layer_expression_thresholds(_region) against the unfused sequence: bit for bit."""
import numpy as np
import pytest

from tests.ref_py import pointwise_ref as P
from tests.user_layer_cases import SHAPES, WEIGHTED, context, grid, holed, rects, same

pytestmark = pytest.mark.gpu
SCORES = ("traversability_slope", "traversability_step", "traversability_roughness")
STEPS = [("lower", 0.3, 0.0), ("upper", 0.7, 1.0), ("lower", 0.0, np.nan), ("upper", 0.5, np.inf)]


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    return capi


def special(rows, cols, batch, seed):
    """holes, +-0.0, +-inf and the thresholds themselves"""
    a = holed(rows, cols, batch, seed, -1.0, 2.0)
    flat = a.reshape(-1)
    flat[5:13] = np.array([0.0, -0.0, np.inf, -np.inf, 0.3, 0.7, 0.5, np.float32(0.3)], np.float32)
    return a


@pytest.mark.parametrize("rows, cols, batch", SHAPES)
@pytest.mark.parametrize("layer", ["mine", "traversability_step"])
def test_threshold_and_copy(capi, rows, cols, batch, layer):
    a = special(rows, cols, batch, 1)
    with context(capi, rows, cols, batch) as ctx:
        ctx.add_layer("mine")
        for mode, thr, set_to in STEPS:
            ctx.upload_layer(layer, a)
            ctx.run_threshold(layer, mode, thr, set_to)
            assert same(ctx.download(layer), P.threshold(a, mode, thr, set_to)), (mode, thr)
        # one map of the batch: the others keep their bits (the run starts at any 16-byte phase: rows * cols is odd at 37 x 29)
        ctx.upload_layer(layer, a)
        ctx.run_threshold(layer, "upper", 0.7, -2.0, batch - 1, 1)
        want = a.copy()
        want[batch - 1] = P.threshold(a[batch - 1], "upper", 0.7, -2.0)
        assert same(ctx.download(layer), want)
        for m in range(batch):
            for r0, c0, h, w in rects(rows, cols):
                ctx.upload_layer(layer, a)
                ctx.run_threshold_region(layer, "lower", 0.3, 9.0, m, r0, c0, h, w)
                want = a.copy()
                want[m] = P.threshold_region(a[m], "lower", 0.3, 9.0, r0, c0, h, w)
                assert same(ctx.download(layer), want), (m, r0, c0, h, w)
        # DuplicationFilter: into a layer without memory, one map only, onto itself
        ctx.upload_layer(layer, a)
        dup = ctx.add_layer("dup")
        ctx.copy_layer(layer, dup, batch - 1, 1)
        got = grid(ctx, dup)
        assert same(got[batch - 1], P.copy(a[batch - 1])) and (batch == 1 or np.isnan(got[0]).all())
        ctx.copy_layer(layer, "dup")
        ctx.copy_layer("dup", "dup")
        assert same(ctx.download("dup"), a)
        for call, code in [(lambda: ctx.run_threshold(layer, 3, 0.0, 0.0), capi.TE_ERR_INVALID_ARG),
                           (lambda: ctx.run_threshold(layer, "lower", np.nan, 0.0), capi.TE_ERR_INVALID_ARG),
                           (lambda: ctx.run_threshold(ctx.add_layer("absent"), "lower", 0.0, 0.0), capi.TE_ERR_NOT_READY),
                           (lambda: ctx.run_threshold(25, "lower", 0.0, 0.0), capi.TE_ERR_INVALID_ARG),
                           (lambda: ctx.copy_layer("absent", "dup"), capi.TE_ERR_NOT_READY),
                           (lambda: ctx.copy_layer(layer, 25), capi.TE_ERR_INVALID_ARG),
                           (lambda: ctx.run_threshold(layer, "lower", 0.0, 0.0, batch, 1), capi.TE_ERR_INVALID_ARG)]:
            with pytest.raises(capi.TeError) as e:
                call()
            assert e.value.code == code, str(e.value)


@pytest.mark.parametrize("rows, cols, batch", SHAPES)
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_fused_equals_the_sequence(capi, rows, cols, batch, n):
    lay = {k: holed(rows, cols, batch, 10 + i, 0.0, 1.0) for i, k in enumerate(SCORES)}
    text = WEIGHTED + " + minOfFinites(traversability_step)" if n == 3 else WEIGHTED  # (n = 3: the reduction's code moves up)
    with context(capi, rows, cols, batch) as ctx:
        ctx.add_layer("fused"), ctx.add_layer("steps")
        for k, v in lay.items():
            ctx.upload_layer(k, v)
        ctx.run_layer_expression(text, "fused", thresholds=STEPS[:n])
        ctx.run_layer_expression(text, "steps")
        for mode, thr, set_to in STEPS[:n]:
            ctx.run_threshold("steps", mode, thr, set_to)
        got = ctx.download("fused")
        assert same(got, ctx.download("steps"))
        assert (got == np.float32(STEPS[0][2])).any()  # (a threshold took effect)
        if n != 3:
            r0, c0, h, w = rects(rows, cols)[4]
            old = holed(rows, cols, batch, 99)
            for name in ("fused", "steps"):
                ctx.upload_layer(name, old)
            ctx.run_layer_expression_region(text, "fused", batch - 1, r0, c0, h, w, thresholds=STEPS[:n])
            ctx.run_layer_expression_region(text, "steps", batch - 1, r0, c0, h, w)
            for mode, thr, set_to in STEPS[:n]:
                ctx.run_threshold_region("steps", mode, thr, set_to, batch - 1, r0, c0, h, w)
            assert same(ctx.download("fused"), ctx.download("steps"))
            assert not same(ctx.download("fused"), old)


def test_a_text_at_the_instruction_limit_falls_back(capi):
    rows, cols, batch = SHAPES[0]
    a = holed(rows, cols, batch, 5, 0.0, 0.1)
    text = " + ".join(["traversability_slope"] * 31)  # 61 instructions: three thresholds fit, four do not
    with context(capi, rows, cols, batch) as ctx:
        ctx.add_layer("out")
        ctx.upload_layer("traversability_slope", a)
        assert capi.expr_check(text)["n_instructions"] == 61
        ctx.run_layer_expression(text, "out", thresholds=STEPS[:3])
        fused3 = ctx.download("out")
        with pytest.raises(capi.TeError) as e:
            ctx.run_layer_expression(text, "out", thresholds=STEPS[:4])
        assert e.value.code == capi.TE_ERR_BAD_PARAM and "64 instructions" in str(e.value)
        assert same(ctx.download("out"), fused3)  # the refused call wrote nothing
        # the caller's fallback: the calls one by one
        ctx.run_layer_expression(text, "out")
        for mode, thr, set_to in STEPS[:4]:
            ctx.run_threshold("out", mode, thr, set_to)
        with np.errstate(all="ignore"):
            s = a.copy()
            for _ in range(30):
                s = (s + a).astype(np.float32)
        assert same(ctx.download("out"), P.thresholds(s, STEPS[:4]))
