"""The plan of te_run_distance (csrc/te_distance_plan.h) and its per-cell routines (csrc/te_distance.h) on the CPU:
tests/cpu/distance_plan_check.cpp checks the cap against its defining loop, the rectangles of the region call by single-seed flips,
the owners of every cell under the launch geometry, and column_nearest / row_min against brute force -- plain and, as a
stand-alone program, under the sanitizers; and every case of tests/distance_cases.py takes the route its GPU test claims, the tall
ones their segments and the region cases their rectangles as well."""
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
    assert len(f) == 20, f
    return dict(route=f[0], cap2=int(f[1]), R=int(f[2]), lds=int(f[3]), p1_blocks=int(f[4]), p2_blocks=int(f[5]), seg_chunks=int(f[6]),
                out_rect=tuple(int(v) for v in f[7:11]), p1_segs=int(f[11]), g_rect=tuple(int(v) for v in f[12:16]), in_rect=tuple(int(v) for v in f[16:20]))


@pytest.mark.parametrize("rows,cols,reach,opt,claim", K.ROUTE_CLAIMS)
def test_gpu_cases_take_the_route_they_claim(exe, rows, cols, reach, opt, claim):
    p = route(exe, rows, cols, K.cap_for(reach), opt)
    assert p["route"] == claim and p["R"] == reach
    assert p["cap2"] == D.cap_cells(K.cap_for(reach), K.RES)[0]
    assert p["p2_blocks"] == -(-rows // 64) * -(-cols // 64)
    assert (p["lds"] == K.staged_bytes(cols, reach)) if claim == "tiled" else p["lds"] == 0


@pytest.mark.parametrize("rows,cols,reach,opt,claim,lds,seg_chunks,p1_segs", K.TALL_CASES)
def test_tall_cases_take_the_route_and_the_segments_they_claim(exe, rows, cols, reach, opt, claim, lds, seg_chunks, p1_segs):
    p = route(exe, rows, cols, K.cap_for(reach), opt)
    assert p["route"] == claim and p["R"] == reach
    assert p["cap2"] == D.cap_cells(K.cap_for(reach), K.RES)[0]
    assert p["p2_blocks"] == -(-rows // 64) * -(-cols // 64)
    assert p["lds"] == (K.staged_bytes(cols, reach) if claim == "tiled" else 0)
    if lds is not None:
        assert p["lds"] == lds
    if seg_chunks is not None:
        assert (p["seg_chunks"], p["p1_segs"]) == (seg_chunks, p1_segs)
        assert p["p1_segs"] > 1 and (p1_segs - 1) * seg_chunks * 64 < rows <= p1_segs * seg_chunks * 64
        assert p["p1_blocks"] == p1_segs * -(-cols // 4)
    assert p["out_rect"] == p["g_rect"] == p["in_rect"] == (0, 0, rows, cols)


def test_the_lds_limit_is_met_exactly_and_the_plan_route_turns_at_its_reach(exe):
    by = {(r, c, reach, opt): (claim, lds) for (r, c, reach, opt, claim, lds, _s, _n) in K.TALL_CASES}
    assert by[(3, 600, 224, 1)] == ("tiled", 64 * 1024) and by[(3, 600, 225, 1)] == ("any", 0) and by[(3, 600, 224, 0)] == ("any", 0)
    assert by[(70, 200, 64, 0)][0] == "tiled" and by[(70, 200, 65, 0)][0] == "any"
    assert K.staged_bytes(600, 224) == 64 * 1024 and K.staged_bytes(600, 225) > 64 * 1024


@pytest.mark.parametrize("name", sorted(K.REGION_TALL))
def test_tall_region_cases_have_the_rectangles_they_claim(exe, name):
    case = K.REGION_TALL[name]
    (rows, cols), reach = case["shape"], case["reach"]
    for opt in (0, 1):
        whole = route(exe, rows, cols, K.cap_for(reach), opt)
        assert whole["seg_chunks"] == case["seg_chunks"] and whole["p1_segs"] > 1
        for (r0, c0, h, w), claim in case["rects"]:
            p = route(exe, rows, cols, K.cap_for(reach), opt, (r0, c0, h, w))
            i0, j0, i1, j1 = max(0, r0 - reach), max(0, c0 - reach), min(rows, r0 + h + reach), min(cols, c0 + w + reach)
            assert p["out_rect"] == (i0, j0, i1 - i0, j1 - j0)
            assert p["g_rect"][0] == i0 and p["g_rect"][2] == i1 - i0 and p["in_rect"][0] == max(0, i0 - reach)
            if "out" in claim:
                assert p["out_rect"] == claim["out"]
            if "g_i0" in claim:
                assert (p["g_rect"][0], p["in_rect"][0]) == (claim["g_i0"], claim["in_i0"])
            if "p1_segs" in claim:
                assert (p["seg_chunks"], p["p1_segs"]) == (claim["plan_seg_chunks"], claim["p1_segs"])
            assert p["route"] == ("tiled" if opt == 1 or reach <= 64 else "any")
    # case A's first rectangle: its g starts inside a chunk, and its pre-halo is two chunks of which in.i0 masks a part
    claim = K.REGION_TALL["A"]["rects"][0][1]
    assert claim["g_i0"] % 64 != 0 and 64 < claim["g_i0"] - claim["in_i0"] <= 128 and (claim["g_i0"] - claim["in_i0"]) % 64 != 0


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
