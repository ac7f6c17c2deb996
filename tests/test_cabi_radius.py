"""The symbols of te_run_radius_filter and the argument checks that need no device."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    return capi


def test_symbols_are_exported(capi):
    L = capi.load()
    for name in ("te_run_radius_filter", "te_radius_filter_stats", "te_time_radius_filter_samples"):
        assert name in capi.SYMBOLS and hasattr(L, name)
    assert (capi.RADIUS_MEAN, capi.RADIUS_MIN, capi.OPT_RADIUS_ROUTE) == (1, 2, 11)


def test_the_header_declares_them(capi):
    import os
    from tests.conftest import ROOT
    text = open(os.path.join(ROOT, "include", "travgpu.h")).read()
    for want in ("#define TE_RADIUS_MEAN 1", "#define TE_RADIUS_MIN 2", "#define TE_OPT_RADIUS_ROUTE 11",
                 "int te_run_radius_filter(te_ctx* ctx, int op, double radius, int in_layer, int out_layer, int map0, int nmaps);",
                 "int te_radius_filter_stats(te_ctx* ctx, uint64_t counts[2]);"):
        assert want in text, want


def test_null_and_bad_arguments_are_rejected_without_a_device(capi):
    L = capi.load()
    counts = (C.c_uint64 * 2)()
    out = (C.c_float * 4)()
    assert L.te_run_radius_filter(None, 1, 0.1, 0, 0, 0, 1) == capi.TE_ERR_INVALID_ARG
    assert b"te_run_radius_filter" in L.te_last_error()
    assert L.te_radius_filter_stats(None, counts) == capi.TE_ERR_INVALID_ARG
    assert b"te_radius_filter_stats" in L.te_last_error()
    assert L.te_time_radius_filter_samples(None, 1, 0.1, 0, 3, 0, 1, out) == capi.TE_ERR_INVALID_ARG
