"""The route of the circular footprint pass, decided by the library's OWN code: tests/cpu/fp_route_check.cpp
is compiled from traversability_estimation_amd/csrc/te_fp_route.h -- the header launch_footprint routes with -- and builds
its inputs from te_fp_table.h, the tables the shim builds.  Every footprint row of DESIGN.md 4.7 is pinned by a named case
here; a seeded sweep holds every route to what its kernels rely on (2R+1 <= 31 and a list that holds the reservations for
k_fp_slide5, whole-cell ties for k_fp_slide4, k >= 17 for both, a map one wavefront wide and under 4 GiB, an instantiated
shape).  A test that declines silently no longer sends a map to a slower kernel unnoticed: rows = 65 and 4033 did until
round 5."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

# name: (route, k_fp_blocked follows)
CASES = {
    "cfg3": ("slide5", 1),                               # 4096^2, tie-free R = 9, the layer the chain wrote
    "cfg3_any_reach_option": ("any", 0),                 # TE_OPT_FP_ANY_REACH = 1
    "reference_045_at_003": ("slide4", 1),               # the reference's 0.45 m at 0.03 m: a whole-cell tie radius of 15 cells
    "reference_045_at_003_uploaded": ("general", 0),     # ... on an uploaded layer (no bound: tcap < 0)
    "tie_free_9_uploaded": ("slide3", 0),                # tie-free <= 16 on an uploaded layer
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
    got = {}
    for line in r.stdout.split("\n"):
        if line:
            name, route, k, strip_rows, chunk, blocked = line.split()
            got[name] = (route, int(blocked))
            if route in ("slide4", "slide5"):
                assert int(k) >= 17 and 1 <= int(strip_rows) <= 512 and int(chunk) in (64, 128, 256), line
    assert got == CASES


@pytest.mark.parametrize("seed", [1, 2])
def test_sweep_holds_every_route_to_its_kernels(exe, seed):
    r = subprocess.run([exe, "sweep", "3000", str(seed)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "3000 cases, 0 failed checks" in r.stdout
    counts = dict(kv.split() for kv in r.stdout.split("routes: ")[1].split("\n")[0].split(", "))
    assert all(int(v) > 0 for v in counts.values()), counts  # (every route is exercised)
