"""te_upload_layer_tile, te_run_median_fill_region and te_run_radius_filter_region: declared in include/travgpu.h with the
documented signatures, exported by the library, bound by capi (no GPU needed: NULL arguments are refused before any device
call)."""
import ctypes as C
import os
import re

from tests.conftest import ROOT

SIGNATURES = {
    "te_upload_layer_tile": "int te_upload_layer_tile(te_ctx* ctx, int layer, const float* host_tile, int map, int row0, int col0, int h, int w);",
    "te_run_median_fill_region": "int te_run_median_fill_region(te_ctx* ctx, const te_median_fill_params* p, int in_layer, int out_layer, int map, int row0, "
                                 "int col0, int h, int w, int out_rect[4]);",
    "te_run_radius_filter_region": "int te_run_radius_filter_region(te_ctx* ctx, int op, double radius, int in_layer, int out_layer, int map, int row0, int col0, "
                                   "int h, int w, int out_rect[4]);",
}


def test_the_header_declares_the_documented_signatures():
    with open(os.path.join(ROOT, "include", "travgpu.h")) as f:
        text = re.sub(r"\s+", " ", f.read())
    for name, sig in SIGNATURES.items():
        assert re.sub(r"\s+", " ", sig) in text, name


def test_the_library_exports_them_and_capi_binds_them():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    lib = capi.load()
    ip = C.POINTER(C.c_int)
    assert lib.te_upload_layer_tile.argtypes == [C.c_void_p, C.c_int, C.POINTER(C.c_float)] + [C.c_int] * 5
    assert lib.te_run_median_fill_region.argtypes == [C.c_void_p, C.POINTER(capi.TeMedianFillParams)] + [C.c_int] * 7 + [ip]
    assert lib.te_run_radius_filter_region.argtypes == [C.c_void_p, C.c_int, C.c_double] + [C.c_int] * 7 + [ip]
    for name in SIGNATURES:
        assert name in capi.SYMBOLS
    for method in ("upload_layer_tile", "run_median_fill_region", "run_radius_filter_region"):
        assert callable(getattr(capi.Context, method))
    # NULL is refused with TE_ERR_INVALID_ARG and a message that names the call, before anything touches a device
    rect = (C.c_int * 4)()
    assert lib.te_upload_layer_tile(None, 3, None, 0, 0, 0, 1, 1) == capi.TE_ERR_INVALID_ARG
    assert b"te_upload_layer_tile" in lib.te_last_error()
    assert lib.te_upload_layer_tile(None, 0, None, 0, 0, 0, 1, 1) == capi.TE_ERR_INVALID_ARG  # (the elevation: te_upload_tile's own refusal)
    assert lib.te_run_median_fill_region(None, None, 0, 1, 0, 0, 0, 1, 1, rect) == capi.TE_ERR_INVALID_ARG
    assert b"te_run_median_fill_region" in lib.te_last_error()
    assert lib.te_run_radius_filter_region(None, 1, 0.1, 0, 1, 0, 0, 0, 1, 1, rect) == capi.TE_ERR_INVALID_ARG
    assert b"te_run_radius_filter_region" in lib.te_last_error()
