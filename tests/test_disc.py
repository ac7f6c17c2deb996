"""The host tables the kernels take their shape from, built by the library's OWN code: tests/cpu/disc_check.cpp is compiled
from traversability_estimation_amd/csrc/te_disc.h (build_disc, the tie circle, the tie summary of the footprint route, the
clip table of border moments) and te_fp_table.h (footprint_inner_q, the inner rings of the route of any reach) -- the headers
the shim builds and uploads its tables from -- and holds them to brute force over the cells, membership decided in the check
itself by di^2 + dj^2 against (radius / res)^2 and the tie tolerance.  Once plain, once under AddressSanitizer and
UndefinedBehaviorSanitizer (the builders write fixed arrays of 33 runs and 32 ties)."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpu", "disc_check.cpp")
INC = os.path.join(ROOT, "traversability_estimation_amd", "csrc")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_disc_tables_against_brute_force(tmp_path, flags):
    exe = str(tmp_path / "disc_check")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + flags + ["-I", INC, SRC, "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    checks, failed = (int(v) for v in r.stdout.split("\n")[-2].split()[0:4:2])
    assert checks > 50000 and failed == 0, r.stdout[-2000:]
