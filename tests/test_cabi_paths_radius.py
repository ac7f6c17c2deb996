"""te_check_footprint_paths_radius at the C-ABI boundary, without a GPU: the library exports it, the header declares it, it
rejects bad arguments before it touches a device, and capi.Context carries the method."""
import ctypes as C
import inspect

import pytest


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    return capi


def test_symbol_is_exported_and_bound(capi):
    L = capi.load()
    assert hasattr(L, "te_check_footprint_paths_radius")
    assert "te_check_footprint_paths_radius" in capi.SYMBOLS
    assert C.sizeof(capi.TePathCheckStats) == 3 * C.sizeof(C.c_int)
    sig = inspect.signature(capi.Context.check_footprint_paths_radius)
    assert list(sig.parameters) == ["self", "paths", "radii", "offset", "map_index", "want_stats"]
    assert sig.parameters["offset"].default == 0.15 and sig.parameters["map_index"].default == 0
    assert sig.parameters["want_stats"].default is False


def test_bad_arguments_are_rejected_without_a_device(capi):
    L = capi.load()
    off = (C.c_int * 2)(0, 1)
    xy = (C.c_double * 2)(0.0, 0.0)
    rad = (C.c_double * 1)(0.3)
    safe, trav, st = (C.c_ubyte * 1)(), (C.c_double * 1)(), (C.c_int * 1)()
    assert L.te_check_footprint_paths_radius(None, 0, 1, off, xy, rad, 0.15, safe, trav, st, None) == capi.TE_ERR_INVALID_ARG
    assert b"te_check_footprint_paths_radius" in L.te_last_error()
    # (negative or non-finite radii and offsets: tests/test_gpu_paths_radius.py, on a real context)
    assert L.te_check_footprint_paths_radius(None, 0, 0, None, None, None, 0.15, None, None, None, None) == capi.TE_ERR_INVALID_ARG
