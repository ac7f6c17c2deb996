"""The C-ABI of the user layers, the layer expressions and the point-wise filters: the symbols exist, and the paths that need
no device return the stated codes."""
import ctypes as C
import re
import os

import pytest

from tests.conftest import ROOT

NEW = ["te_add_layer", "te_remove_layer", "te_layer_id", "te_layer_name", "te_expr_check_ctx", "te_run_layer_expression",
       "te_run_layer_expression_region", "te_run_threshold", "te_run_threshold_region", "te_copy_layer", "te_run_layer_expression_thresholds",
       "te_run_layer_expression_thresholds_region"]


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    return capi


def test_symbols_are_declared_bound_and_exported(capi):
    header = open(os.path.join(ROOT, "include", "travgpu.h")).read()
    L = capi.load()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.SYMBOLS and hasattr(L, name), name
    assert "#define TE_MAX_USER_LAYERS 16" in header and capi.MAX_USER_LAYERS == 16 and capi.LAYER_COUNT == 15
    assert C.sizeof(capi.TeThreshold) == 24


def test_null_arguments_are_refused_without_a_device(capi):
    L = capi.load()
    lid = C.c_int(-1)
    buf = C.create_string_buffer(64)
    t = capi.TeThreshold(mode=capi.THRESHOLD_LOWER, threshold=0.0, set_to=0.0)
    calls = [lambda: L.te_add_layer(None, b"a", C.byref(lid)), lambda: L.te_remove_layer(None, 15), lambda: L.te_layer_id(None, b"a", C.byref(lid)),
             lambda: L.te_layer_name(None, 0, buf, 64), lambda: L.te_expr_check_ctx(None, b"1", None), lambda: L.te_run_layer_expression(None, b"1", 4),
             lambda: L.te_run_layer_expression_region(None, b"1", 4, 0, 0, 0, 1, 1), lambda: L.te_run_threshold(None, 4, 1, 0.0, 0.0, 0, 1),
             lambda: L.te_run_threshold_region(None, 4, 1, 0.0, 0.0, 0, 0, 0, 1, 1), lambda: L.te_copy_layer(None, 0, 4, 0, 1),
             lambda: L.te_run_layer_expression_thresholds(None, b"1", 4, 1, C.byref(t)),
             lambda: L.te_run_layer_expression_thresholds_region(None, b"1", 4, 1, C.byref(t), 0, 0, 0, 1, 1)]
    for call in calls:
        assert call() == capi.TE_ERR_INVALID_ARG
        assert b"NULL" in L.te_last_error()


def test_expr_check_without_a_context_does_not_know_user_names(capi):
    with pytest.raises(capi.TeError) as e:
        capi.expr_check("elevation_filled + 1")
    assert e.value.code == capi.TE_ERR_BAD_PARAM and "unknown name" in str(e.value)
