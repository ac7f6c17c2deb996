"""The plan of te_run_distance (csrc/te_distance_plan.h) and its per-cell routines (csrc/te_distance.h) on the CPU:
tests/cpu/distance_plan_check.cpp checks the cap against its defining loop, the rectangles of the region call by single-seed flips,
the owners of every cell under the launch geometry, and column_nearest / row_min against brute force -- plain and, as a
stand-alone program, under the sanitizers; and every case of tests/distance_cases.py takes the route its GPU test claims."""
import os
import subprocess

import pytest

from tests import distance_cases as K
from tests.conftest import ROOT
from tests.ref_py import distance_ref as D

SRC = os.path.join(ROOT, "tests", "cpu", "distance_plan_check.cpp")
INC = os.path.join(ROOT, "traversability_estimation_amd", "csrc")


def build(tmp, flags):
    exe = str(tmp / "distance_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", INC, SRC, "-o", exe], check=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("distance_plan"), ["-O2"])


def out(exe, *args):
    r = subprocess.run([exe] + [repr(a) if isinstance(a, float) else str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout.strip()


def test_plan_program(exe):
    assert ", 0 failed checks" in out(exe)


def test_plan_program_under_the_sanitizers(tmp_path):
    assert ", 0 failed checks" in out(build(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


def route(exe, rows, cols, max_distance, opt, rect=()):
    f = out(exe, "route", rows, cols, float(max_distance), K.RES, opt, *rect).split()
    if f[0] == "refused":
        return None
    return dict(route=f[0], cap2=int(f[1]), R=int(f[2]), lds=int(f[3]), p1_blocks=int(f[4]), p2_blocks=int(f[5]), seg_chunks=int(f[6]),
                out_rect=tuple(int(v) for v in f[7:11]))


@pytest.mark.parametrize("rows,cols,reach,opt,claim", K.ROUTE_CLAIMS)
def test_gpu_cases_take_the_route_they_claim(exe, rows, cols, reach, opt, claim):
    p = route(exe, rows, cols, K.cap_for(reach), opt)
    assert p["route"] == claim and p["R"] == reach
    assert p["cap2"] == D.cap_cells(K.cap_for(reach), K.RES)[0]
    assert p["p2_blocks"] == -(-rows // 64) * -(-cols // 64)
    assert (p["lds"] == K.staged_bytes(cols, reach)) if claim == "tiled" else p["lds"] == 0


def test_the_cap_is_the_reference_s(exe):
    for md in (0.5, 0.15, 0.37, 2.0, 10.0, 1e-9, 1638.0):
        p = route(exe, 10, 10, md, 0)
        assert (p["cap2"], p["R"]) == D.cap_cells(md, K.RES), md
    assert route(exe, 10, 10, 32768 * K.RES, 0) is None and route(exe, 10, 10, 0.0, 0) is None


def test_region_rectangles_are_the_rectangle_grown_by_the_reach(exe):
    rows, cols = K.REGION_SHAPE
    for reach in K.REGION_REACHES:
        for (r0, c0, h, w) in K.rects(rows, cols):
            p = route(exe, rows, cols, K.cap_for(reach), 0, (r0, c0, h, w))
            i0, j0, i1, j1 = max(0, r0 - reach), max(0, c0 - reach), min(rows, r0 + h + reach), min(cols, c0 + w + reach)
            assert p["out_rect"] == (i0, j0, i1 - i0, j1 - j0)
