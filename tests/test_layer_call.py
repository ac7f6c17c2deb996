"""The call contract of the layer filters (csrc/te_layer_call.h) on the CPU: tests/cpu/layer_call_check.cpp compares every verdict
-- over all layer ids, the facts of a context that matter and the map ranges -- with the rules restated as a table, plain and,
as a stand-alone program, under the sanitizers.  The refusals the GPU tests assert (test_refusals of test_gpu_median_fill,
test_gpu_radius_filter and test_gpu_window_expression) are among its cases."""
import os
import subprocess

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpu", "layer_call_check.cpp")
INC = [os.path.join(ROOT, "traversability_estimation_amd", "csrc"), os.path.join(ROOT, "include")]


def build(tmp, flags):
    exe = str(tmp / "layer_call_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + [a for d in INC for a in ("-I", d)] + [SRC, "-o", exe], check=True, timeout=300)
    return exe


def out(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout.strip()


def test_contract_program(tmp_path):
    assert out(build(tmp_path, ["-O2"])).endswith(", 0 failed checks")


def test_contract_program_under_the_sanitizers(tmp_path):
    assert out(build(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])).endswith(", 0 failed checks")
