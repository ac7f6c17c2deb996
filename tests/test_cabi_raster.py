"""TE_OPT_NORMALS_ALGORITHM without a device: the state transition te_set_option runs (te_ctx_state.h: normals_algorithm_set,
plain C++ compiled from the header the shim uses), the option's place in the header and its Python mirror."""
import os
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("raster_state") / "raster_state_check"
    src = os.path.join(ROOT, "tests", "cpu", "raster_state_check.cpp")
    inc = [os.path.join(ROOT, "traversability_estimation_amd", "csrc"), os.path.join(ROOT, "include")]
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", inc[0], "-I", inc[1], src, "-o", str(out)], check=True, timeout=300)
    return str(out)


def test_setting_the_algorithm_drops_results_and_kept_normals(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " checks, 0 failed" in r.stdout and int(r.stdout.split(" checks")[0].split("\n")[-1]) >= 12


def test_the_header_and_the_mirror_agree():
    from traversability_estimation_amd import capi
    text = open(os.path.join(ROOT, "include", "travgpu.h")).read()
    assert "#define TE_OPT_NORMALS_ALGORITHM 13" in text and capi.OPT_NORMALS_ALGORITHM == 13
    assert "restated, not pinned" in text.split("#define TE_OPT_NORMALS_ALGORITHM 13")[0].split("#define TE_OPT_WINDOW_EXPR_ROUTE 12")[1]
    options = [v for k, v in vars(capi).items() if k.startswith("OPT_")]
    assert len(options) == len(set(options)), "two options share a number"


def test_a_null_context_is_rejected_without_a_device():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    L = capi.load()
    assert L.te_set_option(None, capi.OPT_NORMALS_ALGORITHM, 1) == capi.TE_ERR_INVALID_ARG
    assert b"te_set_option" in L.te_last_error()
