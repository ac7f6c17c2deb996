"""The symbols of te_run_components / te_run_reachable / te_components_stats and the argument checks that need no device."""
import ctypes as C
import os
import re

import pytest


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    return capi


NAMES = ("te_run_components", "te_run_reachable", "te_components_stats")


def test_symbols_are_exported(capi):
    L = capi.load()
    for name in NAMES:
        assert name in capi.SYMBOLS and hasattr(L, name)
    assert (capi.COMPONENTS_CONNECTIVITY_4, capi.COMPONENTS_CONNECTIVITY_8, capi.REACHABLE_MAX_STARTS) == (4, 8, 256)
    for method in ("run_components", "run_reachable", "components_stats"):
        assert callable(getattr(capi.Context, method))


def test_the_header_declares_them_and_its_constants_are_capi_s(capi):
    from tests.conftest import ROOT
    text = open(os.path.join(ROOT, "include", "travgpu.h")).read()
    for want in ("int te_run_components(te_ctx* ctx, int mode, double threshold, int connectivity, int in_layer, int out_layer, int map0, int nmaps);",
                 "int te_run_reachable(te_ctx* ctx, int mode, double threshold, int connectivity, int in_layer, int out_layer, int map, int n_starts, "
                 "const int* start_cells /* row, col pairs */);",
                 "int te_components_stats(te_ctx* ctx, uint64_t counts[4]);"):
        assert want in text, want
    defines = {k: int(v, 0) for k, v in re.findall(r"#define (TE_(?:COMPONENTS|REACHABLE|OPT_COMPONENTS)_[A-Z0-9_]+) (0x[0-9a-fA-F]+|\d+)", text)}
    assert defines == {"TE_COMPONENTS_CONNECTIVITY_4": capi.COMPONENTS_CONNECTIVITY_4, "TE_COMPONENTS_CONNECTIVITY_8": capi.COMPONENTS_CONNECTIVITY_8,
                       "TE_REACHABLE_MAX_STARTS": capi.REACHABLE_MAX_STARTS}
    # the limits stand with the contract
    block = text.split("---- Connected regions")[1].split("int te_components_stats")[0]
    for phrase in ("no region form", "no chain-file type", "no C++ plugin", "labels themselves are not exposed", "next float above r"):
        assert phrase in block, phrase


def test_null_and_bad_arguments_are_rejected_without_a_device(capi):
    L = capi.load()
    counts = (C.c_uint64 * 4)()
    one = (C.c_int * 2)(0, 0)
    many = (C.c_int * (2 * 257))()
    ok = capi.DISTANCE_BELOW | capi.DISTANCE_NAN_IS_SEED

    def refused(rc, *words):
        assert rc == capi.TE_ERR_INVALID_ARG
        msg = L.te_last_error()
        for w in words:
            assert w in msg, (w, msg)

    refused(L.te_run_components(None, ok, 0.5, 4, 4, 3, 0, 1), b"te_run_components", b"NULL")
    refused(L.te_run_components(None, ok, 0.5, 5, 4, 3, 0, 1), b"te_run_components", b"connectivity 5")
    refused(L.te_run_components(None, 3, 0.5, 4, 4, 3, 0, 1), b"te_run_components", b"mode 3")
    refused(L.te_run_components(None, 0, 0.5, 8, 4, 3, 0, 1), b"mode 0")
    refused(L.te_run_components(None, capi.DISTANCE_BELOW | capi.DISTANCE_TIME_PASS1, 0.5, 8, 4, 3, 0, 1), b"mode")
    refused(L.te_run_reachable(None, ok, 0.5, 8, 4, 3, 0, 1, one), b"te_run_reachable", b"NULL")
    refused(L.te_run_reachable(None, ok, 0.5, 6, 4, 3, 0, 1, one), b"te_run_reachable", b"connectivity 6")
    refused(L.te_run_reachable(None, 8, 0.5, 4, 4, 3, 0, 1, one), b"te_run_reachable", b"mode 8")
    refused(L.te_run_reachable(None, ok, 0.5, 4, 4, 3, 0, 0, one), b"n_starts 0")
    refused(L.te_run_reachable(None, ok, 0.5, 4, 4, 3, 0, 257, many), b"n_starts 257")
    refused(L.te_run_reachable(None, ok, 0.5, 4, 4, 3, 0, 1, None), b"start_cells is NULL")
    refused(L.te_components_stats(None, counts), b"te_components_stats")
    assert L.te_run_components(None, ok, float("nan"), 4, 4, 3, 0, 1) == capi.TE_ERR_BAD_PARAM
