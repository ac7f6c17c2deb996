"""The route of the circular footprint pass, decided by the library's OWN code: tests/cpu/fp_route_check.cpp
is compiled from traversability_estimation_amd/csrc/te_fp_route.h -- the header launch_footprint routes with -- and builds
its inputs from te_fp_table.h, the tables the shim builds.  Every footprint row of DESIGN.md 4.7 is pinned by a named case
here; a seeded sweep holds every route to what its kernels rely on (2R+1 <= 31 and a list that holds the reservations for
k_fp_slide5, whole-cell ties for k_fp_slide4, k >= 17 for both, a map one wavefront wide and under 4 GiB, an instantiated
shape, and for the two double kernels, which pack the untraversable count into the disc sum, a bound that keeps
npoints * cap under kFpUOff / 2).  The cases of tests/test_gpu_footprint_values.py are pinned here too, with their k
(tests/footprint_value_cases.py).  A test that declines silently no longer sends a map to a slower kernel unnoticed: rows = 65 and 4033 did until
round 5."""
import os
import subprocess

import pytest

from tests import footprint_value_cases as fv
from tests.conftest import ROOT

# name: (route, k_fp_blocked follows)
CASES = {
    "cfg3": ("slide5", 1),                               # 4096^2, tie-free R = 9, the layer the chain wrote
    "cfg3_any_reach_option": ("any", 0),                 # TE_OPT_FP_ANY_REACH = 1
    "reference_045_at_003": ("slide4", 1),               # the reference's 0.45 m at 0.03 m: a whole-cell tie radius of 15 cells
    "reference_045_at_003_uploaded": ("any", 0),         # ... on an uploaded layer (no bound: tcap < 0): no packed sum
    "tie_free_9_uploaded": ("any", 0),                   # tie-free <= 16 on an uploaded layer: likewise
    "tie_free_16": ("slide3", 0),                        # the tie-free 16-cell radius (2R+1 > 31)
    "reach_18": ("general", 0),                          # reach 17 .. 20
    "reach_20_tie": ("general", 0),
    "non_whole_tie_radius": ("general", 0),              # ties off the axis circle (sqrt(50) cells)
    "rows_48": ("general", 0),                           # narrower than a wavefront
    "cells_2_30": ("general", 0),                        # 32-bit byte offsets end at 2^30 cells
    "reach_22_default_yaml_002": ("any", 0),             # above 20 cells
    "reach_45_default_yaml_001": ("any", 0),
    "rows_65": ("slide5", 1),                            # the shifted last block column: still the fixed-point kernels
    "rows_4033": ("slide5", 1),
    "rows_65_tie_15": ("slide4", 1),
    "rows_4033_tie_15": ("slide4", 1),
    "cfg4_512_maps_of_512": ("slide5", 1),               # a batch of 512 maps
    "cfg5_tile_256_of_8192": ("slide5", 1),              # a 256^2 region run of an 8192^2 map
    "zero_rmin": ("slide5", 0),                          # radiusMin = 0: the march writes the blocked discs' 0 itself
    "no_guard_rows": ("slide3", 0),                      # a layer without the slab's guard rows
}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("fp_route") / "fp_route_check"
    src = os.path.join(ROOT, "tests", "cpu", "fp_route_check.cpp")
    inc = os.path.join(ROOT, "traversability_estimation_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", inc, src, "-o", str(out)], check=True,
                   timeout=300)
    return str(out)


def test_named_cases_take_their_rows_of_the_design(exe):
    r = subprocess.run([exe, "cases"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got, got_fv = {}, {}
    for line in r.stdout.split("\n"):
        if line:
            name, route, k, strip_rows, chunk, blocked = line.split()
            if name.startswith("fv_"):
                got_fv[name] = (route, int(k))
            else:
                got[name] = (route, int(blocked))
            if route in ("slide4", "slide5"):
                assert int(k) >= 17 and 1 <= int(strip_rows) <= 512 and int(chunk) in (64, 128, 256), line
    assert got == CASES
    assert got_fv == fv.PLANNED  # the cases of tests/test_gpu_footprint_values.py: route and k


def test_fixed_k_restatement_matches_the_harness(exe):
    """fv.fp_fixed_k -- the three lines the GPU test takes its tolerance 2^-(k+1) from -- gives the k the harness prints,
    at every saturation case: both sides of every step from 23 down to 16."""
    r = subprocess.run([exe, "cases"], capture_output=True, text=True, timeout=120)
    printed = {ln.split()[0]: (ln.split()[1], int(ln.split()[2])) for ln in r.stdout.split("\n") if ln.startswith("fv_sat")}
    assert len(printed) == 27
    for geo, (cells, limit, _, _) in fv.SAT.items():
        for k in range(23, 15, -1):
            tcap = fv.sat_scale(geo, k) * 3.0
            assert fv.fp_fixed_k(cells, fv.fixed_cap(tcap, tcap), limit) == k, (geo, k)
            route, kk = printed[f"fv_{geo}_k{k}"]
            assert (kk == k) if k >= 17 else (kk == -1 and route not in ("slide4", "slide5")), (geo, k, route, kk)
        assert fv.fp_fixed_k(cells, fv.fixed_cap(0.3, fv.sat_scale(geo, 17) * 3.0), limit) == 17 == printed[f"fv_{geo}_defcap"][1]
    assert fv.disc_cells("sat5") == fv.SAT["sat5"][0] and fv.disc_cells("r15") == 709 and fv.disc_cells("reach18") == 1085


def test_restated_constant_is_the_header_s(exe):
    """fv.K_UOFF, from which the GPU test's boundary family takes its two constants, is te_fp_route.h's kFpUOff."""
    r = subprocess.run([exe, "constants"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    printed = dict(ln.split() for ln in r.stdout.split("\n") if ln)
    assert float(printed["kFpUOff"]) == fv.K_UOFF


@pytest.mark.parametrize("seed", [1, 2])
def test_sweep_holds_every_route_to_its_kernels(exe, seed):
    r = subprocess.run([exe, "sweep", "3000", str(seed)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "3000 cases, 0 failed checks" in r.stdout
    counts = dict(kv.split() for kv in r.stdout.split("routes: ")[1].split("\n")[0].split(", "))
    assert all(int(v) > 0 for v in counts.values()), counts  # (every route is exercised)
