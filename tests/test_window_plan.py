"""The plan of te_run_window_expression (csrc/te_window_plan.h) on the CPU: tests/cpu/window_plan_check.cpp checks rule 2, the
ownership of the cells, the LDS figure and the route decisions, plain and -- as a stand-alone program -- under the sanitizers;
and every shape, window and expression of tests/window_expression_cases.py lands on the route its GPU test claims."""
import os
import subprocess

import pytest

from tests import window_expression_cases as K
from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpu", "window_plan_check.cpp")
INC = os.path.join(ROOT, "traversability_estimation_amd", "csrc")


def build(tmp, flags):
    exe = str(tmp / "window_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", INC, SRC, "-o", exe], check=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("window_plan"), ["-O2"])


def out(exe, *args):
    r = subprocess.run([exe] + [repr(a) if isinstance(a, float) else str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout.strip()


def route(exe, rows, cols, w, edge, reductions, outer, option):
    """-> (route of the call, the tile is staged, workgroups per map on the separable route, workgroups that walk directly)"""
    kind, staged, _lds, sep, direct = out(exe, "route", rows, cols, w, K.EDGES.index(edge), reductions, outer, option).split()
    return kind, staged == "1", int(sep), int(direct)


def off_lds_window(exe):
    return int(out(exe, "offlds"))


def test_plan_program(exe):
    assert ", 0 failed checks" in out(exe)


def test_plan_program_under_the_sanitizers(tmp_path):
    assert ", 0 failed checks" in out(build(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


@pytest.mark.parametrize("length,res,w", [(0.05, 0.03, 3), (0.1, 0.05, 3), (0.15, 0.05, 3), (0.025, 0.05, 1), (0.02, 0.05, 1), (0.25, 0.05, 5)])
def test_window_length(exe, length, res, w):
    assert out(exe, "size", 0, 1, length, res) == str(w)


def test_window_size_refusals(exe):
    for ws in (0, 2, 4, -1):
        assert out(exe, "size", ws, 0, 0.0, 0.05).startswith("ERR")
    for length in (-0.05, float("nan"), float("inf")):
        assert out(exe, "size", 0, 1, length, 0.05).startswith("ERR")


def test_gpu_cases_take_the_route_they_claim(exe):
    off = off_lds_window(exe)
    assert off > max(K.WINDOWS)
    for rows, cols, _batch in K.SHAPES:
        for w in K.WINDOWS + [off]:
            for _text, reductions, outer in K.EXACT:
                for option in (0, 1, 2):
                    for edge in K.EDGES:
                        kind, staged, sep, direct = route(exe, rows, cols, w, edge, reductions, outer, option)
                        want = "direct" if w == off else K.claim(reductions, outer, w, option)
                        assert kind == want, (rows, cols, w, edge, reductions, outer, option)
                        assert staged == (w != off)
                        assert sep + direct == -(-rows // 32) * -(-cols // 8)
                        if kind == "direct":
                            assert sep == 0
                        elif edge != "mean":
                            assert direct == 0
                        else:  # only the workgroups none of whose windows is clipped
                            assert (sep, direct) == whole_window_tiles(rows, cols, w), (rows, cols, w, sep, direct)


def whole_window_tiles(rows, cols, w):
    """(tiles of 32 x 8 cells none of whose windows reaches beyond the map, the other tiles)"""
    m = (w - 1) // 2
    whole = sum(1 for i0 in range(0, rows, 32) for j0 in range(0, cols, 8)
                if i0 - m >= 0 and min(i0 + 31, rows - 1) + m <= rows - 1 and j0 - m >= 0 and min(j0 + 7, cols - 1) + m <= cols - 1)
    return whole, -(-rows // 32) * -(-cols // 8) - whole


def test_mean_padding_keeps_interior_workgroups_separable(exe):
    # 130 x 33 at w = 3: the tiles at rows 32, 64, 96 and columns 8, 16, 24 have whole windows
    assert route(exe, 130, 33, 3, "mean", 1, 0, 1)[2:] == (9, 16)
    assert route(exe, 130, 33, 3, "crop", 1, 0, 1)[2:] == (25, 0)
    assert route(exe, 130, 33, 3, "crop", 1, 0, 0)[2:] == (0, 25)  # by plan a window of 3 walks directly
    assert route(exe, 130, 33, 5, "crop", 1, 0, 0)[2:] == (25, 0)
    assert route(exe, 130, 33, 3, "mean", 3, 1, 1)[2:] == (0, 25)
