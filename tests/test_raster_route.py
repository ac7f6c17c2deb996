"""The route plan of the filter chain under NormalVectorsFilter's raster method (te_chain_route.h, ChainRouteIn::raster), without
a GPU: tests/cpu/raster_route_check.cpp runs the header the launchers route with.

With `raster` set: never a one-kernel route, always kNormalsRaster, the roughness stage plan_filter_route(kFilterRoughness)
gives, the steps and the combine as under area.  Without it: every field of every plan as the header of the commit before the
raster method gave it (tests/golden/raster_route/area_plans.txt: one hash per swept input, whole maps, regions and per-plugin
plans; the check program's own header comment says how the file was made)."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "raster_route", "area_plans.txt")
N_AREA, SEED_AREA = 2000, 7


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("raster_route") / "raster_route_check"
    src = os.path.join(ROOT, "tests", "cpu", "raster_route_check.cpp")
    inc = [os.path.join(ROOT, "traversability_estimation_amd", "csrc"), os.path.join(ROOT, "include")]
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", inc[0], "-I", inc[1], src, "-o", str(out)], check=True, timeout=300)
    return str(out)


@pytest.mark.parametrize("seed", [11, 12])
def test_raster_plans(exe, seed):
    r = subprocess.run([exe, "raster", "3000", str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "3000 cases, 0 failed checks" in r.stdout
    cover = dict(kv.split("=") for kv in r.stdout.split("coverage: ")[1].split())
    # every roughness route, the normals alone, both combines and both stream forms were planned
    assert all(int(v) >= 20 for v in cover.values()), cover


def test_area_plans_are_the_parents(exe):
    r = subprocess.run([exe, "area", str(N_AREA), str(SEED_AREA)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(GOLDEN) as f:
        want = f.read().split("\n")
    got = r.stdout.split("\n")
    assert len(want) == N_AREA + 1 and len(got) == len(want)
    moved = [k for k, (a, b) in enumerate(zip(got, want)) if a != b]
    if moved:
        full = subprocess.run([exe, "area", str(N_AREA), str(SEED_AREA), "full"], capture_output=True, text=True, timeout=120).stdout.split("\n")
        assert not moved, "plans that differ from the parent's:\n" + "\n".join(full[k] for k in moved[:8])


def test_the_sweep_of_area_plans_reaches_every_kind(exe):
    """What the golden file stands for: whole maps, regions and the three per-plugin plans, the one-kernel routes included."""
    full = subprocess.run([exe, "area", str(N_AREA), str(SEED_AREA), "full"], capture_output=True, text=True, timeout=120).stdout
    lines = [ln for ln in full.split("\n") if ln]
    assert len(lines) == N_AREA
    for words in ("filter=0 whole=0", "filter=0 whole=1", "filter=2 ", "filter=3 ", "filter=5 "):
        assert sum(words in ln for ln in lines) >= 100, words
    # the plan's own `whole` (a one-kernel route), and the normals kernels bar the slim and sparse marches of k_normals3, which
    # need a radius of 9 or 10 cells on a map without (with few) holes: a handful of the inputs at most
    for field in [" whole=1 sh", " whole=2 sh"] + [f" normals={k} " for k in (0, 3, 4, 5, 6, 7, 8, 9)]:
        assert any(field in ln for ln in lines), field
