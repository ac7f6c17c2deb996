"""te_run_layer_expression(_region) on the device: into `traversability` it IS te_run_expression, bits and state; into a user
layer and into a score layer it equals the numpy contract (tests/ref_py/expression_ref.py) bit for bit on texts without
transcendental functions; the region form writes the whole-map call's bits on the rectangle and nothing else."""
import numpy as np
import pytest

from tests.ref_py import expression_ref as E
from tests.user_layer_cases import SHAPES, WEIGHTED, context, grid, holed, rects, same

pytestmark = pytest.mark.gpu
SCORES = ("traversability_slope", "traversability_step", "traversability_roughness")
# no transcendental function: + - * / sqrt abs square cwiseMin / cwiseMax are exact in float32 on both sides
TEXTS = [WEIGHTED, "cwiseMin(traversability_slope, traversability_step) - abs(traversability_roughness) ./ 3",
         "sqrt(square(traversability_slope) + square(traversability_step)) / maxOfFinites(traversability_roughness)"]


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    return capi


def scores(rows, cols, batch, seed):
    return {k: holed(rows, cols, batch, seed + i, 0.0, 1.0) for i, k in enumerate(SCORES)}


@pytest.mark.parametrize("rows, cols, batch", SHAPES)
def test_into_traversability_is_te_run_expression(capi, rows, cols, batch):
    lay = scores(rows, cols, batch, 10)
    elev = np.random.default_rng(3).uniform(0.0, 0.3, (batch, cols, rows)).astype(np.float32)
    with context(capi, rows, cols, batch) as A, context(capi, rows, cols, batch) as B:
        for ctx in (A, B):
            ctx.upload_elevation(elev)
            ctx.run_chain(capi.RUN_FOOTPRINT)
            for k, v in lay.items():
                ctx.upload_layer(k, v)
        A.run_expression(TEXTS[1])
        B.run_layer_expression(TEXTS[1], "traversability")
        assert same(A.download("traversability"), B.download("traversability"))
        # the state calls that follow behave alike: the footprint pass reads the new values on the route of any reach
        for ctx in (A, B):
            ctx.run_footprint()
        assert same(A.download("traversability_footprint"), B.download("traversability_footprint"))
        A.run_expression_region(WEIGHTED, 0, 3, 4, 9, 7)
        B.run_layer_expression_region(WEIGHTED, "traversability", 0, 3, 4, 9, 7)
        assert same(A.download("traversability"), B.download("traversability"))
        for ctx in (A, B):
            ctx.run_chain_region(0, 3, 4, 9, 7, capi.RUN_FOOTPRINT)
        for k in ("traversability", "traversability_footprint"):
            assert same(A.download(k), B.download(k)), k


@pytest.mark.parametrize("rows, cols, batch", SHAPES)
@pytest.mark.parametrize("out", ["mine", "traversability_slope"])
def test_equals_the_numpy_contract(capi, rows, cols, batch, out):
    lay = scores(rows, cols, batch, 20)
    with context(capi, rows, cols, batch) as ctx:
        ctx.add_layer("mine")
        for text in TEXTS:
            for k, v in lay.items():
                ctx.upload_layer(k, v)
            ctx.run_layer_expression(text, out)  # (traversability_slope: in place, the text reads it)
            assert E.same_bits(grid(ctx, out), E.evaluate(text, lay)), text
        # a user layer as an operand: the bits of the same text over a reference layer that holds the same values
        ctx.upload_layer("mine", lay["traversability_step"])
        ctx.upload_layer("traversability_slope", lay["traversability_slope"])
        ctx.run_layer_expression("(mine + traversability_slope) / 2 - mine .* mine", ctx.add_layer("second"))
        want = E.evaluate("(traversability_step + traversability_slope) / 2 - traversability_step .* traversability_step", lay)
        assert E.same_bits(grid(ctx, "second"), want)
        info = ctx.expr_check("mine + second")
        assert info["layer_mask"] == (1 << ctx.layer_id("mine")) | (1 << ctx.layer_id("second")) and info["layers"] == ["mine", "second"]


def test_refusals(capi):
    rows, cols, batch = SHAPES[0]
    with context(capi, rows, cols, batch) as ctx:
        ctx.add_layer("mine"), ctx.add_layer("absent")
        for k in SCORES:
            ctx.upload_layer(k, holed(rows, cols, batch, 1))
        for call, code in [(lambda: ctx.run_layer_expression("absent + 1", "mine"), capi.TE_ERR_NOT_READY),
                           (lambda: ctx.run_layer_expression("nobody + 1", "mine"), capi.TE_ERR_BAD_PARAM),
                           (lambda: ctx.run_layer_expression(WEIGHTED, 20), capi.TE_ERR_INVALID_ARG),   # never added
                           (lambda: ctx.run_layer_expression(WEIGHTED, 31), capi.TE_ERR_INVALID_ARG),
                           (lambda: ctx.run_layer_expression(WEIGHTED, "traversability_x"), capi.TE_ERR_INVALID_ARG),  # no memory yet
                           (lambda: ctx.run_layer_expression_region("meanOfFinites(traversability_slope)", "mine", 0, 0, 0, 2, 2), capi.TE_ERR_UNSUPPORTED),
                           (lambda: ctx.run_layer_expression_region(WEIGHTED, "mine", 0, 0, 0, rows + 1, 2), capi.TE_ERR_INVALID_ARG)]:
            with pytest.raises(capi.TeError) as e:
                call()
            assert e.value.code == code, str(e.value)
        ctx.run_layer_expression(WEIGHTED, "mine")
        with pytest.raises(capi.TeError) as e:  # in place on a rectangle
            ctx.run_layer_expression_region("mine + 1", "mine", 0, 0, 0, 2, 2)
        assert e.value.code == capi.TE_ERR_UNSUPPORTED
        ctx.run_layer_expression("mine + 1", "mine")  # ... and fine on whole maps
        # the old entry point keeps its contract
        with pytest.raises(capi.TeError) as e:
            ctx.run_expression(WEIGHTED, "traversability_slope")
        assert e.value.code == capi.TE_ERR_INVALID_ARG


@pytest.mark.parametrize("rows, cols, batch", SHAPES)
@pytest.mark.parametrize("out", ["mine", "traversability_footprint"])
def test_region_form(capi, rows, cols, batch, out):
    lay = scores(rows, cols, batch, 30)
    old = holed(rows, cols, batch, 40)
    text = TEXTS[1]
    with context(capi, rows, cols, batch) as ctx:
        ctx.add_layer("mine"), ctx.add_layer("whole")
        for k, v in lay.items():
            ctx.upload_layer(k, v)
        ctx.run_layer_expression(text, "whole")
        whole = grid(ctx, "whole")
        for m in range(batch):
            for r0, c0, h, w in rects(rows, cols):
                ctx.upload_layer(out, old)
                ctx.run_layer_expression_region(text, out, m, r0, c0, h, w)
                want = old.copy()
                want[m, c0:c0 + w, r0:r0 + h] = whole[m, c0:c0 + w, r0:r0 + h]
                assert same(ctx.download(out), want), (m, r0, c0, h, w)
