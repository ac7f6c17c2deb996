"""The route of the filter chain, decided by the library's OWN code: tests/cpu/chain_route_check.cpp is
compiled from traversability_estimation_amd/csrc/te_chain_route.h -- the header launch_chain and launch_filter route with --
on the discs of te_disc.h and the hole hints of te_hole_routing.h.  Every chain row of DESIGN.md 4.7 is pinned by a named
case here; a seeded sweep holds every route to what its kernels rely on (the launchers' former early returns, each stated
once) and reaches every value of every route field; and the kernel names in the ids of tests/test_gpu_conditioning.py are
the plan's.  The same program runs once more under ASan / UBSan, stand-alone."""
import os
import subprocess

import numpy as np
import pytest

from tests import conditioning_cases as cc
from tests.conftest import ROOT

# name: (one-kernel chain, step height, step score, normals kernel, k_normals_fixup follows, combine, two streams)
CASES = {
    "cfg3": ("none", "march<81>", "march<81>", "k_normals3s", 1, "k_combine", 1),  # 4096^2, tie-free R = 9, hole-free, not kept
    "cfg3_footprint": ("none", "march<81>", "march<81>", "k_normals3s", 1, "deferred", 1),  # ... the mask kernel combines
    "cfg3_speckle_0.1%": ("none", "march<81>", "march<81>", "k_normals3-sparse", 1, "k_combine", 1),
    "cfg3_speckle_5%": ("none", "march<81>", "march<81>", "k_normals3-dense", 1, "k_combine", 1),
    "cfg3_regions": ("none", "march<81>", "march<81>", "k_normals3-dense-short", 1, "k_combine", 1),  # runs >= 8 cells: short strips
    "cfg3_kept": ("none", "march<81>", "march<81>", "k_normals3-KEEP-dense", 1, "k_combine", 1),
    "cfg3_sequential": ("none", "march<81>", "march<81>", "k_normals3s", 1, "k_combine", 0),  # TE_RUN_SEQUENTIAL: no aux stream
    "cfg4_512_maps_of_512_speckle": ("none", "march<25>", "march<25>", "k_normals3-dense", 1, "k_combine", 1),  # more blocks than hole queues
    "tie_3": ("none", "RAW<8>+ties", "RAW<8>+ties", "k_normals3-TIES", 1, "k_combine", 1),
    "tie_4": ("none", "RAW<13>+ties", "RAW<13>+ties", "k_normals3-TIES", 1, "k_combine", 1),
    "tie_10": ("none", "RAW<98>+ties", "RAW<98>+ties", "k_normals3-TIES", 1, "k_combine", 1),
    # the default YAML at res 0.05: a one-cell tie radius (CROSS) and single-cell step windows -- one kernel at every size
    # (tie discs take k_normals_small whatever the launch's size; only tie-free discs stop at 2^18 cells)
    "default_yaml_005_4096": ("k_normals_small+step+combine", "-", "-", "-", 0, "in_chain", 0),
    "default_yaml_005_1024": ("k_normals_small+step+combine", "-", "-", "-", 0, "in_chain", 0),
    "bag_map_100x133_003": ("k_chain_window", "-", "-", "-", 0, "in_chain", 0),
    "default_yaml_005_2^18": ("k_chain_window", "-", "-", "-", 0, "in_chain", 0),
    "default_yaml_005_2^18+64": ("k_normals_small+step+combine", "-", "-", "-", 0, "in_chain", 0),
    "tie_free_reach2_2^18+64": ("none", "k_step_small", "k_step_small", "k_normals3-dense", 1, "k_combine", 0),  # not k_normals_small
    "rows_48": ("none", "generic", "generic", "k_normals_slide", 1, "in_normals", 0),
    "rows_64": ("none", "march<25>", "march<25>", "k_normals3-dense", 1, "k_combine", 0),
    "radius_11": ("none", "generic", "generic", "k_normals_slide<R>", 1, "in_normals", 0),
    "radius_16": ("none", "generic", "generic", "k_normals_slide<R>", 1, "in_normals", 0),
    "radius_17": ("none", "generic", "generic", "k_normals", 0, "in_normals", 0),
    "normals_5_roughness_7": ("none", "march<25>", "march<25>", "k_normals", 0, "in_normals", 0),
    "axis_x": ("none", "march<25>", "march<25>", "k_normals", 0, "in_normals", 0),
    "generic_kernels": ("none", "generic", "generic", "k_normals", 0, "k_combine", 1),
    "any_normals": ("none", "march<25>", "march<25>", "any", 0, "in_normals", 0),
    "any_roughness": ("none", "march<25>", "march<25>", "any", 0, "in_normals", 0),
    "any_step1": ("none", "any", "march<25>", "k_normals3-dense", 1, "k_combine", 0),
    "any_step2": ("none", "march<25>", "any", "k_normals3-dense", 1, "k_combine", 0),
    "cells_2^30": ("none", "march<81>", "march<81>", "k_normals_slide", 1, "k_combine", 1),  # k_normals3's 32-bit offsets end at 2^30 cells
    "narrower_than_the_disc": ("none", "march<81>", "march<81>", "k_normals", 0, "in_normals", 0),
    "step_one_cell": ("none", "k_step_small", "k_step_small", "k_normals3-dense", 1, "k_combine", 0),
    "step_tie_1": ("none", "k_step_small", "k_step_small", "k_normals3-dense", 1, "k_combine", 0),
    "step_tie_2": ("none", "k_step_small", "k_step_small", "k_normals3-dense", 1, "k_combine", 0),
    "step_5": ("none", "march<25>", "march<25>", "k_normals3-dense", 1, "k_combine", 0),
    "step_no_guard_rows": ("none", "generic", "generic", "k_normals3-dense", 1, "k_combine", 0),
    "step_region_narrower_than_64": ("none", "generic", "generic", "k_normals_slide", 1, "k_combine", 0),
    "cfg5_tile_256_of_8192": ("none", "march<25>", "march<25>", "k_normals3-dense", 1, "k_combine", 0),  # no one-kernel chain on a region
    "normals_only": ("none", "-", "-", "k_normals3s", 1, "none", 0),
    "filter_slope": ("none", "-", "-", "-", 0, "none", 0),
    "filter_step": ("none", "march<25>", "march<25>", "-", 0, "none", 0),
    "filter_roughness": ("none", "-", "-", "k_normals_slide", 1, "none", 0),  # given normals: the sliding kernel + fix-up
    "filter_combine": ("none", "-", "-", "-", 0, "k_combine", 0),
    "filter_normals": ("none", "-", "-", "k_normals3-KEEP-dense", 1, "none", 0),
    "filter_roughness_tie": ("none", "-", "-", "k_normals", 0, "none", 0),
    "filter_roughness_any": ("none", "-", "-", "any", 0, "none", 0),
    "filter_roughness_16": ("none", "-", "-", "k_normals_slide<R>", 1, "none", 0),
}
CFG5_COMBINE_RECT = (4086, 4086, 4362, 4362)  # the 256^2 tile at (4096, 4096) grown by the chain's reach: both step windows, 5 + 5 cells


def _build(tmp_path_factory, tag, extra):
    out = tmp_path_factory.mktemp(tag) / "chain_route_check"
    src = os.path.join(ROOT, "tests", "cpu", "chain_route_check.cpp")
    inc = os.path.join(ROOT, "traversability_estimation_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + extra + ["-I", inc, src, "-o", str(out)], check=True, timeout=300)
    return str(out)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory, "chain_route", [])


def _cases(out):
    got, rect = {}, None
    for line in out.split("\n"):
        f = line.split()
        if f and f[0] == "cfg5_combine_rect":
            rect = tuple(int(v) for v in f[1:])
        elif f:
            got[f[0]] = (f[1], f[2], f[3], f[4], int(f[5]), f[6], int(f[7]))
    return got, rect


def test_named_cases_take_their_rows_of_the_design(exe):
    r = subprocess.run([exe, "cases"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got, rect = _cases(r.stdout)
    assert got == CASES
    assert rect == CFG5_COMBINE_RECT


@pytest.mark.parametrize("seed", [1, 2])
def test_sweep_holds_every_route_to_its_kernels(exe, seed):
    r = subprocess.run([exe, "sweep", "3000", str(seed)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "3000 cases, 0 failed checks" in r.stdout
    counts = {ln.split(":")[0]: [int(v) for v in ln.split(":")[1].split()] for ln in r.stdout.split("\n") if ":" in ln and not ln.startswith("FAIL")}
    assert {k: len(v) for k, v in counts.items()} == dict(whole=3, step=5, normals=10, combine=5, flags=6)
    assert all(v > 0 for row in counts.values() for v in row), counts  # (every value of every route field occurs)


def _conditioning_line(name, route):
    """What the harness asks of a fixture on a route: the facts of tests/conditioning_cases.py, the invalid cells and their runs
    in memory order as the upload counts them, the step windows of the fixture's parameters.  (A batch + region run is asked as
    its first launch: the whole batch of two maps with the normals kept.)"""
    from tests.test_gpu_conditioning import _fixture
    rows, cols, res, pos, elev, over, rank = _fixture(name, route)
    step = [over.get(k, 0.04) / res for k in ("step_radius1", "step_radius2")]  # (0.04 m: the default of robot_filter_parameter.yaml)
    batch = 2 if route == "batch+region" else 1
    bad = ~np.isfinite(np.asarray(elev).reshape(-1))
    invalid = int(bad.sum())
    runs = int(bad[0]) + int((bad[1:] & ~bad[:-1]).sum())
    clustered = invalid > 0 and runs * 8 <= invalid
    return "%d %d %r %r %d %r %d %d %d %r %r %d" % (rows, cols, res, over["normals_radius"] / res, route != "scores", invalid / bad.size, clustered,
                                                     route == "generic" or rank, route == "any", step[0], step[1], batch)


def test_conditioning_ids_name_the_planned_kernel(exe):
    """tests/test_gpu_conditioning.py names a kernel in every test id (kernel_of): it is the one the plan gives that fixture on
    that route."""
    from tests.test_gpu_conditioning import kernel_of, routes_of
    pairs = [(n, r) for n in cc.names() for r in routes_of(n)]
    r = subprocess.run([exe, "conditioning"], input="\n".join(_conditioning_line(n, rt) for n, rt in pairs) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    planned = r.stdout.split()
    assert len(planned) == len(pairs)
    wrong = [(n, rt, kernel_of(n, rt), p) for (n, rt), p in zip(pairs, planned) if kernel_of(n, rt) != p]
    assert not wrong, wrong


def _plugin_routes(exe):
    """(case, planned route, claimed route) of every case of tests/plugin_filter_cases.py, asked of plan_filter_route."""
    from tests import plugin_filter_cases as K
    r = subprocess.run([exe, "filter"], input="\n".join(K.route_line(c) for c in K.ALL) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    planned = [ln for ln in r.stdout.split("\n") if ln]
    assert len(planned) == len(K.ALL)
    return [(K.case_id(c), c.filter, p, K.route_words(c)) for c, p in zip(K.ALL, planned)]


# the routes the single plugins' GPU tests have to reach, as the `filter` mode prints them
PLUGIN_ROUTES = {2: {"k_step_small", "march<5>", "march<29>", "RAW<8>+ties", "RAW<20>+ties", "generic", "any"},
                 3: {"k_normals_slide", "k_normals_slide<R>", "k_normals", "any"},
                 5: {"k_normals_small-CROSS", "k_normals3-KEEP-dense", "k_normals3-KEEP-TIES", "k_normals_slide<R>", "k_normals"}}


def test_plugin_filter_cases_take_the_routes_they_claim(exe):
    """tests/test_gpu_plugin_filters.py names a route for every case it runs through te_run_filter: it is the one
    plan_filter_route gives that shape, radius, flag and hole count; and between them the cases reach every route of each plugin."""
    rows = _plugin_routes(exe)
    wrong = [r for r in rows if r[2] != r[3]]
    assert not wrong, wrong
    for f, names in PLUGIN_ROUTES.items():
        assert {w for r in rows if r[1] == f for w in r[2].split()} == names, f


def _param_routes(exe):
    """(case, planned route, claimed route) of every case of tests/param_route_cases.py, asked of the chain plan (`params` mode)."""
    from tests import param_route_cases as P
    r = subprocess.run([exe, "params"], input="\n".join(P.route_line(c, P.elevation(c)) for c in P.ALL) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got, _ = _cases(r.stdout)
    assert len(got) == len(P.ALL)  # (the ids are distinct)
    return [(c, got[P.case_id(c)][:6], c.route) for c in P.ALL]


def test_param_route_cases_take_the_routes_they_claim(exe):
    """tests/test_gpu_param_routes.py names a route for every case: it is the one the plan gives that shape, those radii, flags,
    axis and hole counts (a region case: its region launch; the te_run_filter case: TE_FILTER_NORMALS); under axis x / y that is
    never a one-kernel chain and always k_normals."""
    from tests import param_route_cases as P
    rows = _param_routes(exe)
    wrong = [(c.name, p, w) for c, p, w in rows if p != w]
    assert not wrong, wrong
    axis = [(c, p) for c, p, _ in rows if c.axis != 2]
    assert [c for c, _ in axis] == P.AXIS and all(p[0] == "none" and p[3] in ("k_normals", "any") for _, p in axis)


def test_weight_cases_reach_every_combine_and_every_normals_kernel(exe):
    """Between them the weight cases run every kind of combine and every normals kernel that can precede one; and every place
    that writes the weighted sum has its cases, under both weight sets."""
    from tests import param_route_cases as P
    rows = [(c, p) for c, p, _ in _param_routes(exe) if c.axis == 2 and c.gap is None]
    assert [c for c, _ in rows] == P.WEIGHTS
    assert {p[5] for _, p in rows} == P.WEIGHT_COMBINES
    assert {p[0] if p[0] != "none" else p[3] for _, p in rows} == P.WEIGHT_KERNELS
    names = {c.name for c in P.WEIGHTS}
    for site, cases in P.SITES.items():
        assert len(cases) >= 2 and set(cases) <= names, site
        assert {n.rsplit(", ", 1)[1] for n in cases} == {"dyadic weights", "rounding weights"}, site


def test_under_sanitizers(tmp_path_factory):
    """The same program with -fsanitize=address,undefined, stand-alone: the named cases, one sweep, the plugin cases and the
    parameter cases."""
    exe = _build(tmp_path_factory, "chain_route_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([exe, "cases"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert _cases(r.stdout)[0] == CASES
    r = subprocess.run([exe, "sweep", "1000", "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "1000 cases, 0 failed checks" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    wrong = [r for r in _plugin_routes(exe) if r[2] != r[3]]
    assert not wrong, wrong
    wrong = [(c.name, p, w) for c, p, w in _param_routes(exe) if p != w]
    assert not wrong, wrong
