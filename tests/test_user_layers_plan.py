"""The plain C++ behind the user layers, from the library's own headers (tests/cpu/user_layer_check.cpp): the name table of
te_user_layers.h (name rules, lowest free id first, the 17th refusal, add / remove / add), the call contract of te_layer_call.h
with user ids present, absent and never added, and the transition of te_ctx_state.h that keeps every cached result."""
import os
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("user_layers") / "user_layer_check"
    src = os.path.join(ROOT, "tests", "cpu", "user_layer_check.cpp")
    inc = [os.path.join(ROOT, "traversability_estimation_amd", "csrc"), os.path.join(ROOT, "include")]
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", inc[0], "-I", inc[1], src, "-o", str(out)], check=True, timeout=300)
    return str(out)


@pytest.mark.parametrize("what, line", [("names", "names: done"), ("calls", "calls: 9216 checked"), ("state", "state: done")])
def test_group(exe, what, line):
    r = subprocess.run([exe, what], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert line in r.stdout and "\n0 failed checks" in r.stdout


def test_existing_layer_call_harness_still_builds_against_the_header(tmp_path):
    """tests/cpu/layer_call_check.cpp is untouched: with no user layer added the extended check is the old one."""
    out = tmp_path / "layer_call_check"
    src = os.path.join(ROOT, "tests", "cpu", "layer_call_check.cpp")
    inc = [os.path.join(ROOT, "traversability_estimation_amd", "csrc"), os.path.join(ROOT, "include")]
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", inc[0], "-I", inc[1], src, "-o", str(out)], check=True, timeout=300)
