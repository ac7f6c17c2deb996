"""The symbols of te_run_window_expression and the checks that need no device: the header, the NULL arguments, the validation of
te_window_expr_params, and te_window_expr_check."""
import ctypes as C
import os

import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    return capi


NAMES = ("te_window_expr_params_default", "te_window_expr_params_validate", "te_window_expr_check", "te_run_window_expression",
         "te_window_expression_stats", "te_time_window_expression_samples")


def test_symbols_are_exported(capi):
    L = capi.load()
    for name in NAMES:
        assert name in capi.SYMBOLS and hasattr(L, name)
    assert capi.OPT_WINDOW_EXPR_ROUTE == 12
    assert (capi.EDGE_INSIDE, capi.EDGE_CROP, capi.EDGE_EMPTY, capi.EDGE_MEAN) == (0, 1, 2, 3)


def test_the_header_declares_them(capi):
    text = open(os.path.join(ROOT, "include", "travgpu.h")).read()
    for want in ("#define TE_EDGE_INSIDE 0", "#define TE_EDGE_CROP 1", "#define TE_EDGE_EMPTY 2", "#define TE_EDGE_MEAN 3", "#define TE_OPT_WINDOW_EXPR_ROUTE 12",
                 "int te_window_expr_params_default(te_window_expr_params* p);",
                 "int te_window_expr_params_validate(const te_window_expr_params* p);",
                 "int te_window_expr_check(const char* text, int in_layer, te_expr_info* info);",
                 "int te_run_window_expression(te_ctx* ctx, const te_window_expr_params* p, const char* text, int in_layer, int out_layer, int map0, int nmaps);",
                 "int te_window_expression_stats(te_ctx* ctx, uint64_t counts[2]);",
                 "int te_time_window_expression_samples(te_ctx* ctx, const te_window_expr_params* p, const char* text, int in_layer, int out_layer, int warmup, int iters, float* ms);"):
        assert want in text, want
    # the struct of the header and the ctypes mirror: the same fields in the same order, 32 bytes
    body = text[text.index("typedef struct te_window_expr_params {"):text.index("} te_window_expr_params;")]
    assert [f for f, _ in capi.TeWindowExprParams._fields_] == [line.split(";")[0].split()[-1] for line in body.splitlines()[1:] if ";" in line]
    assert C.sizeof(capi.TeWindowExprParams) == 32


def test_null_arguments_name_the_function(capi):
    L = capi.load()
    p = capi.window_expr_params(window_size=3)
    counts = (C.c_uint64 * 2)()
    out = (C.c_float * 4)()
    assert L.te_run_window_expression(None, C.byref(p), b"mean(elevation)", 0, 0, 0, 1) == capi.TE_ERR_INVALID_ARG
    assert b"te_run_window_expression" in L.te_last_error()
    assert L.te_window_expression_stats(None, counts) == capi.TE_ERR_INVALID_ARG
    assert b"te_window_expression_stats" in L.te_last_error()
    assert L.te_time_window_expression_samples(None, C.byref(p), b"mean(elevation)", 0, 3, 0, 1, out) == capi.TE_ERR_INVALID_ARG
    assert b"te_time_window_expression_samples" in L.te_last_error()
    assert L.te_window_expr_check(None, 0, None) == capi.TE_ERR_INVALID_ARG
    assert L.te_window_expr_params_default(None) == capi.TE_ERR_INVALID_ARG
    assert L.te_window_expr_params_validate(None) == capi.TE_ERR_INVALID_ARG


def test_params_defaults_and_validation(capi):
    L = capi.load()
    p = capi.TeWindowExprParams()
    assert L.te_window_expr_params_default(C.byref(p)) == capi.TE_OK
    assert (p.size, p.window_size, p.use_window_length, p.window_length, p.compute_empty_cells, p.edge_handling) == (32, 3, 0, 0.0, 1, capi.EDGE_INSIDE)
    assert L.te_window_expr_params_validate(C.byref(p)) == capi.TE_OK

    def code(**over):
        q = capi.TeWindowExprParams()
        L.te_window_expr_params_default(C.byref(q))
        for k, v in over.items():
            setattr(q, k, v)
        return L.te_window_expr_params_validate(C.byref(q))

    for ws in (0, 2, 4, -1, -3):  # even, zero (neither size nor length), negative
        assert code(window_size=ws) == capi.TE_ERR_BAD_PARAM, ws
        assert b"window_size" in L.te_last_error()
    assert code(window_size=3, use_window_length=1, window_length=0.25) == capi.TE_ERR_BAD_PARAM  # both
    assert b"exactly one" in L.te_last_error()
    assert code(window_size=3, window_length=0.25) == capi.TE_ERR_BAD_PARAM  # both, the length unannounced
    assert code(window_size=0, use_window_length=1, window_length=0.25) == capi.TE_OK
    for bad in (-0.05, float("nan"), float("inf")):
        assert code(window_size=0, use_window_length=1, window_length=bad) == capi.TE_ERR_BAD_PARAM, bad
    for edge in (-1, 4, 17):
        assert code(edge_handling=edge) == capi.TE_ERR_BAD_PARAM, edge
        assert b"edge_handling" in L.te_last_error()
    assert code(size=28) == capi.TE_ERR_INVALID_ARG and code(abi_version=99) == capi.TE_ERR_INVALID_ARG
    for ok in (1, 3, 21, 2147483647):
        assert code(window_size=ok) == capi.TE_OK
    # the Python helper goes through the same validation
    with pytest.raises(capi.TeError):
        capi.window_expr_params(window_size=4)
    with pytest.raises(capi.TeError):
        capi.window_expr_params()
    with pytest.raises(capi.TeError):
        capi.window_expr_params(window_size=3, window_length=0.15)
    assert capi.window_expr_params(window_length=0.15, edge_handling="mean", compute_empty_cells=False).edge_handling == capi.EDGE_MEAN


STD_DEV = "sqrt(sumOfFinites(square(elevation - meanOfFinites(elevation))) ./ numberOfFinites(elevation))"


def test_window_expr_check(capi):
    info = capi.window_expr_check(STD_DEV)
    assert info["n_reductions"] == 3 and info["layers"] == ["elevation"]
    assert capi.window_expr_check("maxOfFinites(traversability) - minOfFinites(traversability)", "traversability")["layers"] == ["traversability"]
    assert capi.window_expr_check("1 + 2")["layers"] == []
    for text, code, column in (("abs(elevation)", capi.TE_ERR_BAD_PARAM, 1), ("sum(mean(sumOfFinites(elevation)))", capi.TE_ERR_BAD_PARAM, 10),
                               ("mean(traversability_step)", capi.TE_ERR_BAD_PARAM, 6), ("sum(elevation * elevation)", capi.TE_ERR_UNSUPPORTED, 15),
                               ("mean(elevation", capi.TE_ERR_BAD_PARAM, 5)):
        with pytest.raises(capi.TeError) as e:
            capi.window_expr_check(text)
        assert e.value.code == code and f"te_window_expr_check: expression, column {column}:" in str(e.value), (text, str(e.value))
    with pytest.raises(capi.TeError) as e:
        capi.window_expr_check("mean(elevation)", 15)
    assert e.value.code == capi.TE_ERR_BAD_PARAM
    # te_expr_check is as it was: no nesting, a map as the result
    with pytest.raises(capi.TeError) as e:
        capi.expr_check("sum(mean(elevation))")
    assert "reductions do not nest" in str(e.value)
    assert capi.expr_check("abs(elevation)")["n_reductions"] == 0
