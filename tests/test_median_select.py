"""The exact selection of the median fill on the CPU: tests/cpu/median_select_check.cpp compiles csrc/te_median.h -- the text the
kernels compile -- and checks the key order against the float order (negatives, denormals, +-0, +-FLT_MAX; +-inf and NaN left
out) and the selection against std::nth_element on 100 000 random bags of 1 .. 225 values drawn from 1 .. 8 distinct ones.  The
same stand-alone program runs once more under AddressSanitizer and UBSan."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpu", "median_select_check.cpp")
INC = os.path.join(ROOT, "traversability_estimation_amd", "csrc")


@pytest.mark.parametrize("flags,n", [(["-O2"], 100000), (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], 100000)],
                         ids=["plain", "asan_ubsan"])
def test_median_select_program(tmp_path, flags, n):
    exe = str(tmp_path / "median_select_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", INC, SRC, "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe, str(n), "7"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert f"{n} random sets, 0 failed checks" in r.stdout
