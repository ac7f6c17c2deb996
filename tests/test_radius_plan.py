"""The plan of te_run_radius_filter (csrc/te_radius_plan.h) on the CPU: tests/cpu/radius_plan_check.cpp checks the predicate of the
sliding Mean against exact sums and the route decisions, plain and -- as a stand-alone program -- under the sanitizers; and every
case of tests/radius_filter_cases.py lands on the kernel its GPU test claims: the route of the call, and for the value kinds which
workgroups pass the predicate."""
import os
import subprocess

import numpy as np
import pytest

from tests import radius_filter_cases as K
from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpu", "radius_plan_check.cpp")
INC = os.path.join(ROOT, "traversability_estimation_amd", "csrc")


def build(tmp, flags):
    exe = str(tmp / "radius_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", INC, SRC, "-o", exe], check=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("radius_plan"), ["-O2"])


def out(exe, *args):
    r = subprocess.run([exe] + [repr(a) if isinstance(a, float) else str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout.strip()


def test_plan_program(exe):
    assert ", 0 failed checks" in out(exe)


def test_plan_program_under_the_sanitizers(tmp_path):
    assert ", 0 failed checks" in out(build(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


def route(exe, op, rows, cols, cells, opt):
    kind, lds, seg, levels, log2n, R, hw0, reach, n_ties, npoints = out(exe, "route", op, rows, cols, float(K.radius_of(cells)), K.RES, opt).split()
    return kind, dict(lds=int(lds), seg=int(seg), levels=int(levels), log2n=int(log2n), R=int(R), hw0=int(hw0), reach=int(reach), n_ties=int(n_ties),
                      npoints=int(npoints))


@pytest.mark.parametrize("op,rows,cols,cells,opt,claim", K.ROUTE_CLAIMS)
def test_gpu_cases_take_the_route_they_claim(exe, op, rows, cols, cells, opt, claim):
    kind, p = route(exe, op, rows, cols, cells, opt)
    assert kind == claim
    assert p["seg"] == min(rows, 64 + 2 * p["hw0"])
    if kind == "slide":
        assert 0 < p["lds"] <= 64 * 1024
    if cells in K.TIE_CELLS:
        assert p["n_ties"] >= 4 and p["reach"] == cells and p["hw0"] == cells - 1
    if cells == 0.0:
        assert p["R"] == -1 and p["n_ties"] == 1


def exponents(a):
    """(emax, emin) over the finite non-zero cells, denormals as -126; None without one."""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32).ravel()
    e = ((b >> 23) & 0xff).astype(np.int64)
    keep = (e != 255) & ((b & 0x7fffffff) != 0)
    if not keep.any():
        return None
    e = np.where(e == 0, -126, e - 127)[keep]
    return int(e.max()), int(e.min())


def workgroups(exe, a, cells):
    """[(provable)] per workgroup of the sliding Mean on map `a`: the predicate over the cells within `reach` of its 64 x 16 centres."""
    rows, cols = a.shape
    kind, p = route(exe, K.MEAN, rows, cols, cells, 1)
    assert kind == "slide"
    verdicts = []
    for i0 in range(0, rows, 64):
        for j0 in range(0, cols, 16):
            ex = exponents(a[max(0, i0 - p["reach"]):i0 + 64 + p["reach"], max(0, j0 - p["reach"]):j0 + 16 + p["reach"]])
            verdicts.append(True if ex is None else out(exe, "free", ex[0], ex[1], p["log2n"]) == "1")
    return verdicts


@pytest.mark.parametrize("kind", K.VALUE_KINDS + ["bag"])
def test_value_kinds_pass_or_fail_the_predicate_as_claimed(exe, kind):
    for rows, cols in K.VALUE_SHAPES:
        for cells in K.VALUE_RADII_CELLS:
            for holes in K.VALUE_HOLES:
                a = K.holey_maps(rows, cols, 1, K.value_seed(rows, cells), [holes], kind)[0]
                v = workgroups(exe, a, cells)
                if kind in K.UNPROVABLE_KINDS:
                    assert not any(v), (kind, rows, cols, cells, holes)
                else:
                    assert all(v), (kind, rows, cols, cells, holes)


def test_block_routing_map_has_workgroups_of_both_kinds(exe):
    a = K.block_routing_map(np.random.default_rng(K.BLOCK_ROUTING_SEED))
    for cells in K.VALUE_RADII_CELLS:
        v = workgroups(exe, a, cells)
        assert v[0] is False and sum(v) == len(v) - 1, (cells, v)


def test_bag_is_provable_at_every_radius_of_the_gpu_tests(exe):
    for rows, cols, _ in K.SHAPES + [K.BIG_WINDOW[:3]]:
        a = K.holey_maps(rows, cols, 1, 3, ["inf_cells"])[0]
        for cells in K.RADII_CELLS + K.TIE_CELLS + ([K.BIG_WINDOW[3]] if rows == 96 else []):
            assert all(workgroups(exe, a, cells)), (rows, cols, cells)


def test_cancel_values_sum_differently_in_another_order():
    """What the predicate is for: on `cancel` the column-wise order gives other bits than the iterator order."""
    a = K.values("cancel", np.random.default_rng(3), 40, 21).astype(np.float64)
    differ = 0
    for i in range(0, 33):
        for j in range(0, 14):
            win = a[i:i + 7, j:j + 7]
            in_order = 0.0
            for v in win.ravel():
                in_order += v
            by_column = 0.0
            for c in range(7):
                s = 0.0
                for v in win[:, c]:
                    s += v
                by_column += s
            differ += in_order != by_column
    assert differ > 0
