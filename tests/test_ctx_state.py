"""The context's validity state (the transition table), run from the library's OWN code: tests/cpu/ctx_state_check.cpp
is compiled from traversability_estimation_amd/csrc/te_ctx_state.h, the header every entry point of the shim keeps the state
with.  CASES is the table's executable form: each named sequence of transitions with the state it must leave, written from
the assignments the entry points made by hand before the header existed (uploads, te_device_ptr, finish_prefetch_locked,
te_set_params, te_set_option, run_chain_locked, run_footprint_locked, run_whole_locked's replay branch, te_run_filter,
te_run_chain_region, te_check_footprint_paths_radius, te_run_expression).

The sweep asserts what those entry points kept between them: footprint_done and mask_done imply chain_done, chain_done
implies have_elev (the only thing that withdraws an elevation, a torn prefetch, drops the results too), no footprint or mask
transition leaves combine_deferred set, a layer from outside has no bound, the face flags are never passed once the
elevation pointer is out, and "layers freed" is the initial state.  NOT an invariant, and not asserted: footprint_done
implies mask_done -- an upload of a score layer drops the mask and leaves the footprint layer complete (the region
contract), and a failed launch can leave combine_deferred set until the next chain, footprint or mask pass.
invalid_runs is reset wherever invalid_cells is (the header's rule; the entry points used to leave it behind on a tile or
pointer, where nothing reads it)."""
import math
import os
import subprocess

import pytest

from tests.conftest import ROOT

NORMALS, MEMO = 0x1c0, 0xe00  # bits TE_LAYER_NORMAL_X .. Z, TE_LAYER_SLOPE_FOOTPRINT .. ROUGHNESS_FOOTPRINT
FRESH = dict(elev=0, chain=0, fp=0, mask=0, defer=0, ext=0, tptr=0, eptr=0, cells=-1, runs=-1, crit=None, rs=0, written=0)
UPLOAD = dict(FRESH, elev=1, cells=12, runs=3, crit=0.07)        # a whole upload, counted, face flags built for 0.07
COMPLETE = dict(UPLOAD, chain=1, fp=1, mask=1, written=MEMO)     # ... and te_run_chain(FOOTPRINT | FOOTPRINT_MEMO)
UNCOUNTED = dict(cells=-1, runs=-1, crit=None)
NO_RESULTS = dict(chain=0, fp=0, mask=0)

# name: the state (crit None: unknown).  The weights of the harness bound the chain's own layer by 0.75.
CASES = {
    "fresh": FRESH,
    "upload": UPLOAD,
    "upload_no_flags": dict(UPLOAD, cells=0, runs=0, crit=None),  # (a context without face flags: the count alone)
    "upload_count_failed": dict(UPLOAD, **UNCOUNTED),
    "complete": COMPLETE,
    "layers_freed": FRESH,
    "geometry_same_shape": dict(COMPLETE, **NO_RESULTS),
    # the region contract: the three flags stay, the counts and the face flags become unknown
    "tile_after_complete": dict(COMPLETE, **UNCOUNTED),
    "tile_first": dict(FRESH, elev=1),
    "elev_pointer_out": dict(COMPLETE, **NO_RESULTS, **UNCOUNTED, eptr=1, written=MEMO | 0x1),
    "elev_pointer_then_upload": dict(COMPLETE, **NO_RESULTS, eptr=1, written=MEMO | 0x1),  # counted again, flags never passed again
    "touch_only": dict(FRESH, written=0x4000),
    "upload_robot_slope": dict(FRESH, rs=1, written=0x4000),
    "ptr_robot_slope": dict(FRESH, rs=0, written=0x4000),         # te_device_ptr does not make it present
    "ptr_robot_slope_declared": dict(FRESH, rs=1, written=0x4000),
    "robot_slope_declared_absent": dict(FRESH, rs=0, written=0x4000),
    "upload_slope_after_complete": dict(COMPLETE, mask=0, written=MEMO | 0x2),
    "ptr_roughness_after_complete": dict(COMPLETE, mask=0, written=MEMO | 0x8),
    "upload_trav_after_complete": dict(COMPLETE, ext=1, tptr=1, written=MEMO | 0x10),
    "upload_footprint_layer": dict(COMPLETE, written=MEMO | 0x20),
    # the bound is known for the pass right behind the whole-map chain only
    "trav_ptr_then_fresh_run": dict(COMPLETE, ext=0, tptr=1, written=MEMO | 0x10),
    "params_fp_radius": dict(COMPLETE, fp=0),
    "params_fp_max_gap": dict(COMPLETE, fp=0, mask=0),
    "params_fp_critical_step": dict(COMPLETE, fp=0, mask=0, crit=None),
    "params_filter_part": dict(COMPLETE, **NO_RESULTS),
    "params_fp_radius_without_chain": UPLOAD,
    "prefetch_elev_failed": dict(COMPLETE, **NO_RESULTS, **UNCOUNTED, elev=0),
    "prefetch_elev_ok": dict(COMPLETE, **NO_RESULTS, cells=5, runs=5),
    "prefetch_elev_ok_count_failed": dict(COMPLETE, **NO_RESULTS, **UNCOUNTED),
    "prefetch_score_ok": dict(COMPLETE, mask=0),
    "prefetch_inputs_failed": dict(COMPLETE, mask=0),              # (slope was among them; nothing else has arrived)
    "prefetch_inputs_ok": dict(COMPLETE, ext=1, tptr=1, rs=1),
    "opt_fp_any_reach": dict(COMPLETE, fp=0),
    "opt_filter_any_radius": dict(COMPLETE, **NO_RESULTS),
    "chain_launch_failed": dict(UPLOAD, defer=1),
    "chain_fp_before_footprint": dict(UPLOAD, chain=1, defer=1),
    "chain_sequential_fp_before_footprint": dict(UPLOAD, chain=1, defer=0),
    "chain_plain": dict(UPLOAD, chain=1),
    "chain_keep_normals": dict(UPLOAD, chain=1, written=NORMALS),
    "chain_drops_normals_after_keep": dict(UPLOAD, chain=1, written=0),
    "chain_normals_only": dict(UPLOAD, chain=1, written=NORMALS),  # (the footprint bits are ignored)
    "chain_fp_no_memo": dict(UPLOAD, chain=1, fp=1, mask=1, written=0),
    "chain_after_external_trav": dict(COMPLETE, fp=0, mask=0, ext=0, tptr=1, written=MEMO | 0x10),
    "run_footprint_after_chain": COMPLETE,
    "region_chain": dict(COMPLETE, fp=0, mask=0),
    "region_chain_fp": COMPLETE,
    "region_chain_fp_after_score_upload": dict(COMPLETE, mask=0, written=MEMO | 0x2),
    "region_keeps_external_and_normals": dict(UPLOAD, chain=1, ext=1, tptr=1, written=NORMALS | 0x10),
    "replay_fp_memo": COMPLETE,
    "replay_plain_after_failed_footprint": dict(UPLOAD, chain=1),
    "filter_slope": dict(COMPLETE, **NO_RESULTS, ext=1),
    "filter_normals": dict(COMPLETE, **NO_RESULTS, ext=1, written=MEMO | NORMALS),
    "filter_then_chain": dict(COMPLETE, fp=0, mask=0),
    "mask_built_after_score_upload": dict(COMPLETE, written=MEMO | 0x2),
    "mask_built_takes_deferred_combine": dict(UPLOAD, chain=1, mask=1),
    "expression": dict(COMPLETE, ext=1, tptr=1, written=MEMO | 0x10),
}

TRANSITIONS = ["layers_freed", "geometry_set", "elevation_replaced", "elevation_counted", "count_unknown", "elevation_tile_written",
               "elevation_pointer_out", "layer_touched", "layer_written", "robot_slope_present", "expression_wrote_traversability",
               "prefetch_joined", "params_changed", "footprint_option_changed", "filter_option_changed", "chain_launching", "chain_launched",
               "footprint_launched", "region_footprint_refreshed", "graph_replayed", "filter_ran", "mask_built"]


def derived(s):
    """What the three questions of the header answer in state `s`: the bound for a pass right behind a whole-map chain, for
    any other pass, and whether the face flags describe the elevation for the critical step in force (0.07)."""
    cap_fresh = -1.0 if s["ext"] else 0.75
    cap = -1.0 if (s["ext"] or s["tptr"]) else 0.75
    return cap_fresh, cap, int(not s["eptr"] and s["crit"] == 0.07)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("ctx_state") / "ctx_state_check"
    src = os.path.join(ROOT, "tests", "cpu", "ctx_state_check.cpp")
    inc = [os.path.join(ROOT, "traversability_estimation_amd", "csrc"), os.path.join(ROOT, "include")]
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", inc[0], "-I", inc[1], src, "-o", str(out)], check=True, timeout=300)
    return str(out)


def test_named_cases_leave_the_states_of_the_table(exe):
    r = subprocess.run([exe, "cases"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = {}
    for line in r.stdout.split("\n"):
        if line:
            name, *fields = line.split()
            got[name] = dict(f.split("=") for f in fields)
    assert sorted(got) == sorted(CASES)
    for name, want in CASES.items():
        g = got[name]
        state = {k: (None if math.isnan(float(g[k])) else float(g[k])) if k == "crit" else int(g[k], 0) for k in FRESH}
        assert state == want, name
        assert (float(g["cap_fresh"]), float(g["cap"]), int(g["ff"])) == derived(want), name


def test_replay_is_the_launches_it_stands_for(exe):
    """For every combination of the six TE_RUN_* bits, from a complete state, one with the traversability pointer out and one
    with a failed launch behind it: graph_replayed leaves what chain_launching, chain_launched and footprint_launched leave,
    which is what the replay branch used to assign by hand (with TE_RUN_NORMALS_ONLY the footprint bits are ignored)."""
    r = subprocess.run([exe, "compose"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "192 combinations, 0 mismatches" in r.stdout


@pytest.mark.parametrize("seed", [1, 2])
def test_sweep_keeps_the_invariants(exe, seed):
    r = subprocess.run([exe, "sweep", "3000", str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "3000 sequences" in r.stdout and " 0 failed checks" in r.stdout
    counts = dict(kv.rsplit(" ", 1) for kv in r.stdout.split("transitions: ")[1].split("\n")[0].split(", "))
    assert sorted(counts) == sorted(TRANSITIONS)
    assert all(int(v) > 0 for v in counts.values()), counts  # (every transition ran)
