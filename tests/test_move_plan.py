"""te_move_map's plan and state transition on the CPU, run from the library's OWN headers: tests/cpu/move_plan_check.cpp is
compiled from csrc/te_move_plan.h and csrc/te_ctx_state.h.  The harness checks the geometry cell by cell (exposed rectangles
disjoint and exactly the cells without a source, trailing lines on the axes that moved); here its plans are compared with the
numpy statement of the contract (tests/ref_py/move_ref.py), the rounding with exact expectations, results_kept with the
tie radii the project's other tests use, and map_moved with the region contract."""
import os
import struct
import subprocess

import pytest

from tests.conftest import ROOT
from tests.ref_py import move_ref

SRC = os.path.join(ROOT, "tests", "cpu", "move_plan_check.cpp")
INC = [os.path.join(ROOT, "traversability_estimation_amd", "csrc"), os.path.join(ROOT, "include")]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("move_plan") / "move_plan_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", INC[0], "-I", INC[1], SRC, "-o", str(out)], check=True, timeout=300)
    return str(out)


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    return r.stdout


def test_every_shift_of_small_maps_matches_the_numpy_contract(exe):
    out = run(exe, "sweep")
    assert " 0 failed checks" in out
    n = 0
    for line in out.split("\n"):
        if not line.startswith("plan "):
            continue
        f = line.split()
        rows, cols, kr, kc, n_rects, all_exposed = map(int, f[1:7])
        got = [(tuple(v[:4]), bool(v[4])) for v in (list(map(int, r.split(","))) for r in f[7:])]
        assert len(got) == n_rects
        assert got == move_ref.rectangles(rows, cols, (kr, kc)), line
        assert bool(all_exposed) == (move_ref.all_exposed(rows, cols, (kr, kc)) and (kr, kc) != (0, 0)), line
        # the reference's own rectangles against its own moved layer: the exposed ones are the NaN cells, each once
        if n % 97 == 0:
            import numpy as np
            cover = np.zeros((cols, rows), int)
            for (r0, c0, h, w), exposed in got:
                if exposed:
                    cover[c0:c0 + w, r0:r0 + h] += 1
            assert (cover == move_ref.exposed_mask(rows, cols, (kr, kc))).all(), line
        n += 1
    assert n == sum((2 * (r + 2) + 1) * (2 * (c + 2) + 1) for r in range(1, 13) for c in range(1, 10))


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


@pytest.mark.parametrize("held,res", [((0.0, 0.0), 1.0), ((500.0, -500.0), 0.03), ((12.3, -7.1), 0.05), ((-3.0, 8.0), 0.5)])
def test_fractions_of_a_cell_round_away_from_zero(exe, held, res):
    lines = [l.split() for l in run(exe, "round", repr(held[0]), repr(held[1]), repr(res)).split("\n") if l.startswith("round ")]
    fracs = [0.0, 0.49, -0.49, 0.5, -0.5, 1.5, -1.5, 2.49, -7.5, 1e-9, 300.5]
    assert len(lines) == len(fracs)
    exact = res in (1.0, 0.5)  # (the request held + f * res is then the exact fraction of a cell)
    want_exact = [0, 0, 0, 1, -1, 2, -2, 2, -8, 0, 301]
    for f, l, w in zip(fracs, lines, want_exact):
        nx, ny = float(l[1]), float(l[2])
        kr, kc, n_rects = int(l[3]), int(l[4]), int(l[7])
        (rr, rc), (px, py) = move_ref.shift_and_position(res, held, (nx, ny))
        assert (kr, kc) == (rr, rc), (f, l)
        assert (int(l[5], 16), int(l[6], 16)) == (bits(px), bits(py)), (f, l)  # held + shift * res, bit for bit
        if exact:
            assert (kr, kc) == (w, -w), (f, l)
        if abs(f) < 0.495:
            assert (kr, kc) == (0, 0) and n_rects == 0, (f, l)
            assert (int(l[5], 16), int(l[6], 16)) == (bits(held[0]), bits(held[1])), (f, l)  # a zero shift: the position stays


def test_results_are_kept_only_without_a_tie_disc(exe):
    out = run(exe, "ties")
    got = {l.split()[1]: int(l.split()[2]) for l in out.split("\n") if l.startswith("ties ")}
    assert got == {"default_0.05": 0,        # normals 0.05 m = one cell: a tie
                   "default_0.03": 0,        # footprint 0.45 m = 15 cells: a tie
                   "tie_free_0.05": 1, "tie_free_0.03": 1, "tie_free_reach_25": 1,
                   "tie_free_raster": 0,     # region runs are refused under raster
                   "footprint_tie_only": 0, "no_params": 0}
    args = [l for l in out.split("\n") if l.startswith("args ")][0].split()[1:]
    assert list(map(int, args)) == [-2, -2, -1, -1, -1]  # BAD_PARAM for the request, INVALID_ARG for the map


@pytest.mark.parametrize("seed", [1, 2])
def test_map_moved_keeps_the_region_contract_or_acts_as_an_upload(exe, seed):
    out = run(exe, "state", 2000, seed)
    assert "2000 sequences" in out and " 0 failed checks" in out
    kept = int(out.split(" steps, ")[1].split()[0])
    assert kept > 100  # (states with chain and footprint results were among them)


def test_harness_under_address_and_undefined_sanitizers(tmp_path):
    """The stand-alone harness (its own main, host code only) under -fsanitize=address,undefined."""
    out = tmp_path / "move_plan_check_san"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC[0], "-I", INC[1], SRC,
                    "-o", str(out)], check=True, timeout=300)
    for args in (["sweep"], ["round", "500.0", "-500.0", "0.03"], ["ties"], ["state", "300", "3"]):
        r = subprocess.run([str(out), *args], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
