"""The plan of te_run_median_fill (csrc/te_median_plan.h) on the CPU: tests/cpu/median_plan_check.cpp checks its invariants, plain
and under the sanitizers; the window radius in cells is compared with Python's int(radius / res) -- the same double division,
truncated --; and every (rows, cols, r) of tests/test_gpu_median_fill.py lands on the kernel its test claims."""
import os
import subprocess

import pytest

from tests import median_fill_cases as K
from tests.conftest import ROOT
from tests.ref_py import median_fill_ref as R

SRC = os.path.join(ROOT, "tests", "cpu", "median_plan_check.cpp")
INC = os.path.join(ROOT, "traversability_estimation_amd", "csrc")


def build(tmp, flags):
    exe = str(tmp / "median_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", INC, SRC, "-o", exe], check=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("median_plan"), ["-O2"])


def out(exe, *args):
    r = subprocess.run([exe] + [repr(a) if isinstance(a, float) else str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout.strip()


def test_plan_program(exe):
    assert ", 0 failed checks" in out(exe)


def test_plan_program_under_the_sanitizers(tmp_path):
    assert ", 0 failed checks" in out(build(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


RADIUS_CASES = [(0.15, 0.05, 2), (0.11, 0.03, 3), (0.04, 0.05, 0), (0.02, 0.03, 0), (0.0, 0.05, 0), (0.05, 0.05, 1), (0.1, 0.05, 2), (0.3, 0.1, 2),
                (0.35, 0.05, None), (0.06, 0.02, None), (0.09, 0.03, None), (1.0, 0.1, None), (0.7, 0.1, None), (2.0, 0.05, None), (12.34, 0.0371, None)]


@pytest.mark.parametrize("radius,res,want", RADIUS_CASES)
def test_radius_in_cells(exe, radius, res, want):
    got = int(out(exe, "radius", radius, res))
    assert got == int(radius / res) == R.radius_cells(radius, res)
    if want is not None:
        assert got == want


def test_radii_of_the_gpu_tests():
    for r in K.RADII + [40, 2]:
        assert R.radius_cells(K.radius_for(r), K.RES) == r


@pytest.mark.parametrize("rows,cols,batch,r,opt,claim", K.ROUTE_CLAIMS)
def test_gpu_cases_take_the_route_they_claim(exe, rows, cols, batch, r, opt, claim):
    route, pr, lds, blocks, tx, ty = out(exe, "route", rows, cols, batch, r, opt).split()
    assert route == claim and int(pr) == r
    if route == "tile":
        assert int(lds) == (64 + 2 * r) * (16 + 2 * r) * 4 + 2048 <= 20 * 1024
        assert int(blocks) == -(-rows // 64) * -(-cols // 16) * batch
