"""te_median_fill_params and the argument checks of te_run_median_fill / te_download_fill_mask that need no device."""
import ctypes as C
import math

import pytest


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    return capi


def test_defaults(capi):
    p = capi.default_median_fill_params()
    assert p.size == C.sizeof(capi.TeMedianFillParams) == 40 and p.abi_version == 1
    assert (p.fill_hole_radius, p.filter_existing_values, p.existing_value_radius, p.num_erode_dilation_iterations) == (0.05, 0, 0.0, 4)
    assert capi.load().te_median_fill_params_validate(C.byref(p)) == capi.TE_OK
    assert capi.load().te_median_fill_params_default(None) == capi.TE_ERR_INVALID_ARG
    with pytest.raises(KeyError):
        capi.default_median_fill_params(radius=1.0)


def test_te_params_is_untouched(capi):
    assert C.sizeof(capi.TeParams) == capi.default_params().size


@pytest.mark.parametrize("field,bad,msg", [("fill_hole_radius", -0.01, "fill_hole_radius"), ("fill_hole_radius", math.nan, "fill_hole_radius"),
                                           ("fill_hole_radius", math.inf, "fill_hole_radius"), ("existing_value_radius", -1.0, "existing_value_radius"),
                                           ("existing_value_radius", math.nan, "existing_value_radius"),
                                           ("num_erode_dilation_iterations", -1, "num_erode_dilation_iterations")])
def test_validation_mirrors_configure(capi, field, bad, msg):
    L = capi.load()
    q = capi.default_median_fill_params(**{field: bad})
    assert L.te_median_fill_params_validate(C.byref(q)) == capi.TE_ERR_BAD_PARAM
    assert msg in L.te_last_error().decode()
    with pytest.raises(capi.TeError) as e:
        capi.validate_median_fill_params(q)
    assert e.value.code == capi.TE_ERR_BAD_PARAM


def test_valid_edges(capi):
    for over in ({"fill_hole_radius": 0.0}, {"num_erode_dilation_iterations": 0}, {"existing_value_radius": 1e9, "filter_existing_values": 1}):
        capi.validate_median_fill_params(capi.default_median_fill_params(**over))


def test_size_and_abi_are_checked(capi):
    L = capi.load()
    q = capi.default_median_fill_params()
    q.size = 8
    assert L.te_median_fill_params_validate(C.byref(q)) == capi.TE_ERR_INVALID_ARG
    q = capi.default_median_fill_params()
    q.abi_version = 99
    assert L.te_median_fill_params_validate(C.byref(q)) == capi.TE_ERR_INVALID_ARG
    assert L.te_median_fill_params_validate(None) == capi.TE_ERR_INVALID_ARG


def test_null_arguments_are_rejected_without_a_device(capi):
    L = capi.load()
    p = capi.default_median_fill_params()
    buf = (C.c_ubyte * 4)()
    out = (C.c_float * 4)()
    assert L.te_run_median_fill(None, C.byref(p), 0, 0, 0, 1) == capi.TE_ERR_INVALID_ARG
    assert b"te_run_median_fill" in L.te_last_error()
    assert L.te_download_fill_mask(None, 0, buf, 4) == capi.TE_ERR_INVALID_ARG
    assert b"te_download_fill_mask" in L.te_last_error()
    assert L.te_time_median_fill_samples(None, C.byref(p), 0, 3, 0, 1, out) == capi.TE_ERR_INVALID_ARG
