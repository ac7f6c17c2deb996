"""The plans of te_run_median_fill_region and te_run_radius_filter_region (csrc/te_region_plan.h) on the CPU:
tests/cpu/region_plan_check.cpp checks, for every rectangle of small maps and for rectangles of maps of several tiles, that
every cell of the output rectangle has exactly one owner on every route, that no launch addresses a cell outside the map, that
every mask stage reads only what the stage before computed, and that the stages give the whole-map mask -- plain and under the
sanitizers.  The rectangles of tests/test_gpu_prefilter_region.py are restated here against the program's output."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpu", "region_plan_check.cpp")
INC = [os.path.join(ROOT, "traversability_estimation_amd", "csrc"), os.path.join(ROOT, "include")]


def build(tmp, flags):
    exe = str(tmp / "region_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + [a for d in INC for a in ("-I", d)] + [SRC, "-o", exe], check=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("region_plan"), ["-O2"])


def out(exe, *args, code=0):
    r = subprocess.run([exe] + [repr(a) if isinstance(a, float) else str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == code, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout.strip()


def test_plan_program(exe):
    assert ", 0 failed checks" in out(exe)


def test_plan_program_under_the_sanitizers(tmp_path):
    assert ", 0 failed checks" in out(build(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


# (rows, cols, r_fill, r_exist, k, option, rect) -> route, reach, out_rect, workgroups
@pytest.mark.parametrize("args,want", [
    ((67, 45, 1, -1, 0, 0, 33, 22, 1, 1), "tile 1 32 21 3 3 1"),
    ((67, 45, 2, -1, 2, 0, 0, 0, 8, 8), "tile 6 0 0 14 14 1"),
    ((131, 70, 2, 1, 2, 1, 123, 62, 8, 8), "tile 6 117 56 14 14 1"),
    ((131, 70, 16, -1, 2, 0, 0, 35, 131, 5), "any 20 0 15 131 45 24"),   # 131 * 45 cells, 256 each
    ((131, 70, 1, -1, 0, 2, 0, 0, 131, 70), "any 1 0 0 131 70 36"),
    ((131, 70, 1, -1, 0, 0, 0, 0, 131, 70), "tile 1 0 0 131 70 15"),      # 3 x 5 tiles of 64 x 16
    ((8192, 8192, 2, -1, 4, 0, 4000, 4000, 256, 256), "tile 10 3990 3990 276 276 90"),  # 5 x 18 tiles: the region's, not the map's 65536
])
def test_median_region_plans(exe, args, want):
    assert out(exe, "median", *args) == want


@pytest.mark.parametrize("args,want", [
    ((1, 67, 45, 0.0, 0.05, 0, 33, 22, 1, 1), "slide 0 33 22 1 1 1 1"),
    ((1, 67, 45, 0.1, 0.05, 0, 0, 0, 8, 8), "slide 2 0 0 10 10 1 1"),
    ((2, 131, 70, 0.45, 0.05, 2, 0, 35, 131, 5), "gather 9 0 26 131 23 3 6"),
    ((1, 131, 70, 0.15, 0.05, 1, 0, 0, 131, 70), "slide 3 0 0 131 70 3 5"),
    ((1, 8192, 8192, 0.075, 0.05, 0, 4000, 4000, 256, 256), "slide 1 3999 3999 258 258 5 17"),
])
def test_radius_region_plans(exe, args, want):
    assert out(exe, "radius", *args) == want


def test_a_rectangle_outside_the_map_is_refused(exe):
    out(exe, "median", 67, 45, 1, -1, 0, 0, 60, 0, 8, 4, code=2)
    out(exe, "radius", 1, 67, 45, 0.1, 0.05, 0, 0, 40, 4, 6, code=2)
