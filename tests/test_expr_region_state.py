"""What te_run_expression_region and te_run_chain_region_expression decide without a device (tests/cpu/expr_region_check.cpp):
the named transition of csrc/te_ctx_state.h, the sequence tile -> one-call tick with and without the footprint flag against
te_run_chain_region + te_upload_layer_tile(traversability) from every start a caller can be in, and the classification of
texts the rectangle form refuses (a reduction, a text that reads the traversability layer) -- plain and, as a stand-alone
program, under the sanitizers.  The public header declares the three entry points and capi binds them."""
import os
import re
import subprocess

import pytest

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpu", "expr_region_check.cpp")
INC = [os.path.join(ROOT, "traversability_estimation_amd", "csrc"), os.path.join(ROOT, "include")]


def build(tmp, flags):
    exe = str(tmp / "expr_region_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + flags + [a for d in INC for a in ("-I", d)] + [SRC, "-o", exe], check=True,
                   timeout=300)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("expr_region"), ["-O2"])


def out(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout.strip()


def test_built_in_checks(exe):
    line = out(exe).splitlines()[-1]
    assert ", 0 failed checks" in line and int(line.split()[0]) > 100, line


def test_built_in_checks_under_the_sanitizers(tmp_path):
    assert ", 0 failed checks" in out(build(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


@pytest.mark.parametrize("text,want", [
    ("cwiseMin(cwiseMin(traversability_slope, traversability_step), traversability_roughness)", "OK region"),
    ("acos(surface_normal_z) + traversability_step", "OK region"),
    ("traversability_slope - meanOfFinites(traversability_slope)", "REFUSED reduction"),
    ("numberOfFinites(elevation) * traversability_step", "REFUSED reduction"),
    ("0.5 * traversability + 0.5 * traversability_step", "REFUSED self"),
    ("traversability_footprint + traversability_x", "OK region"),
])
def test_classification_of_texts(exe, text, want):
    assert out(exe, "classify", text) == want


def test_the_entry_points_are_declared_and_bound():
    with open(os.path.join(ROOT, "include", "travgpu.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "traversability_estimation_amd", "capi.py")) as f:
        capi = f.read()
    for name in ("te_run_window_expression_region", "te_run_expression_region", "te_run_chain_region_expression"):
        assert re.search(r"^int %s\(te_ctx\* ctx," % name, header, re.M), name
        assert '"%s"' % name in capi and "L.%s.argtypes" % name in capi, name
    assert "Limit: te_run_chain_region still recombines" not in header
