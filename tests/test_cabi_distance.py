"""The symbols of te_run_distance and the argument checks that need no device."""
import ctypes as C
import os
import re

import pytest


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    return capi


NAMES = ("te_run_distance", "te_run_distance_region", "te_distance_stats", "te_time_distance_samples")


def test_symbols_are_exported(capi):
    L = capi.load()
    for name in NAMES:
        assert name in capi.SYMBOLS and hasattr(L, name)
    assert (capi.DISTANCE_BELOW, capi.DISTANCE_ABOVE, capi.DISTANCE_NAN_IS_SEED, capi.OPT_DISTANCE_ROUTE) == (1, 2, 4, 14)
    for method in ("run_distance", "run_distance_region", "distance_stats", "time_distance_samples"):
        assert callable(getattr(capi.Context, method))


def test_the_header_declares_them_and_its_constants_are_capi_s(capi):
    from tests.conftest import ROOT
    text = open(os.path.join(ROOT, "include", "travgpu.h")).read()
    for want in ("int te_run_distance(te_ctx* ctx, int mode, double threshold, double max_distance, int in_layer, int out_layer, int map0, int nmaps);",
                 "int te_run_distance_region(te_ctx* ctx, int mode, double threshold, double max_distance, int in_layer, int out_layer, int map, int row0, "
                 "int col0, int h,\n                           int w, int out_rect[4]);",
                 "int te_distance_stats(te_ctx* ctx, uint64_t counts[2]);",
                 "int te_time_distance_samples(te_ctx* ctx, int mode, double threshold, double max_distance, int in_layer, int out_layer, int warmup, "
                 "int iters, float* ms);"):
        assert want in text, want
    defines = {k: int(v, 0) for k, v in re.findall(r"#define (TE_(?:DISTANCE|OPT_DISTANCE)_[A-Z0-9_]+) (0x[0-9a-fA-F]+|\d+)", text)}
    assert defines == {"TE_DISTANCE_BELOW": capi.DISTANCE_BELOW, "TE_DISTANCE_ABOVE": capi.DISTANCE_ABOVE, "TE_DISTANCE_NAN_IS_SEED": capi.DISTANCE_NAN_IS_SEED,
                       "TE_DISTANCE_TIME_PASS1": capi.DISTANCE_TIME_PASS1, "TE_DISTANCE_TIME_PASS2": capi.DISTANCE_TIME_PASS2,
                       "TE_OPT_DISTANCE_ROUTE": capi.OPT_DISTANCE_ROUTE}


def test_null_and_bad_arguments_are_rejected_without_a_device(capi):
    L = capi.load()
    counts = (C.c_uint64 * 2)()
    out = (C.c_float * 4)()
    rect = (C.c_int * 4)()
    assert L.te_run_distance(None, 1, 0.5, 1.0, 4, 3, 0, 1) == capi.TE_ERR_INVALID_ARG
    assert b"te_run_distance" in L.te_last_error()
    assert L.te_run_distance_region(None, 1, 0.5, 1.0, 4, 3, 0, 0, 0, 1, 1, rect) == capi.TE_ERR_INVALID_ARG
    assert b"te_run_distance_region" in L.te_last_error()
    assert L.te_distance_stats(None, counts) == capi.TE_ERR_INVALID_ARG
    assert b"te_distance_stats" in L.te_last_error()
    assert L.te_time_distance_samples(None, 1, 0.5, 1.0, 4, 3, 0, 1, out) == capi.TE_ERR_INVALID_ARG
    assert b"te_time_distance_samples" in L.te_last_error()
