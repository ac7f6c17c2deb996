"""bench.py's surface on the GPU box: every BASELINE configuration is ONE command (`--config cfgK`), the reference's parameter
files are read unchanged (`--yaml`), and each `--full` line carries the contract's keys, a roofline, and a parity check that
passed; a plain line carries the headline alone, and `--dump-outputs` writes what the last timed step computed.
(Short runs: the figures themselves are profiles/r06_configs.json's business.)"""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

KEYS = ("metric", "value", "unit", "n_gpus", "ranks", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config")
FULL_KEYS = ("roofline", "parity_check")


def _bench(*args, env=None, full=True):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args) + (["--full"] if full else []), env=e,
                       capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    for k in KEYS:
        assert k in line, k
    if not full:
        for k in FULL_KEYS + ("latency_ms_per_launch", "host_path", "cpu_baseline", "cpu_baseline_all_cores"):
            assert k not in line, k
        return line
    for k in FULL_KEYS:
        assert k in line, k
    assert line["parity_check"]["ok"] and all(v["mismatches"] == 0 for v in line["parity_check"]["layers"].values())
    rf = line["roofline"]
    assert rf["bound"] == "hbm" and rf["peak"] == 8000.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12
    return line


@pytest.mark.parametrize("cfg,cells,fp", [("cfg1", 100 * 133, False), ("cfg2", 1024 * 1024, False), ("cfg2", 1024 * 1024, True)])
def test_small_configurations_are_one_command(cfg, cells, fp):
    line = _bench("--config", cfg, "--steps", "20", "--warmup", "5", "--cpu-seconds", "2", "--no-cpu-all-cores", *(["--footprint"] if fp else []))
    assert line["config"]["name"] == cfg and line["config"]["map_cells"] == cells and line["config"]["footprint"] is fp
    assert line["cpu_baseline"]["kind"] == "port" and line["cpu_baseline"]["cores"] == 1 and line["cpu_baseline"]["value"] > 0
    assert abs(line["value"] - cells * 20 / (line["ms_per_step"] * 1e-3 * 20)) < 1e-6 * line["value"]
    assert ("traversability_footprint" in line["parity_check"]["layers"]) is fp


def test_streaming_configuration_counts_the_dirty_tile():
    line = _bench("--config", "cfg5", "--steps", "32", "--warmup", "8", "--no-cpu-baseline")
    assert line["config"]["map_cells"] == 8192 * 8192 and line["tick_mode"]["timed"] == "sync" and line["tick_mode"]["stream_ms_per_tick"] > 0
    assert abs(line["value"] - 256 * 256 * line["ticks_per_s"]) < 1e-6 * line["value"]
    assert len(line["parity_check"]["windows"]) == 4  # the windows around the last four tiles


def test_the_references_parameter_values_through_yaml(tmp_path):
    from tests.test_params_yaml import FOOTPRINT, SHIPPED
    f, fp = tmp_path / "robot_filter_parameter.yaml", tmp_path / "robot_footprint_parameter.yaml"
    f.write_text(SHIPPED)
    fp.write_text(FOOTPRINT)
    line = _bench("--yaml", str(f), "--footprint-yaml", str(fp), "--size", "512", "--steps", "20", "--warmup", "5", "--no-cpu-baseline")
    assert "robot_filter_parameter.yaml" in line["config"]["workload"] and abs(line["config"]["radius_cells"] - 1.0) < 1e-9  # 0.05 m on a 0.05 m map
    assert line["parity_check"]["layers"]["traversability_footprint"]["cells"] == 512 * 512


LAYERS = ["traversability_slope", "traversability_step", "traversability_roughness", "traversability", "traversability_footprint"]


def test_a_plain_run_dumps_what_its_last_step_computed(tmp_path, oracle):
    """Without --full: the headline alone.  --dump-outputs: the five layers of the last timed step in float32, the same values
    from run to run (the inputs are seeded), and those of the oracle on the same map."""
    from tests.helpers import compare_layer
    from traversability_estimation_amd import capi, synth
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        line = _bench("--config", "cfg2", "--footprint", "--steps", "7", "--warmup", "2", "--dump-outputs", str(d), full=False)
        assert line["steps"] == 7 and line["warmup"] == 2 and line["config"]["map_cells"] == 1024 * 1024
        assert abs(line["value"] - 1024 * 1024 / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
        assert sorted(os.listdir(d)) == sorted(k + ".npy" for k in LAYERS)
    got = {k: np.load(dirs[0] / (k + ".npy")) for k in LAYERS}
    for k in LAYERS:
        assert got[k].dtype == np.float32 and got[k].shape == (1, 1024, 1024), k
        assert np.array_equal(got[k], np.load(dirs[1] / (k + ".npy")), equal_nan=True), k
    # cfg2's map and parameters, as bench.py builds them
    sys.path.insert(0, ROOT)
    import bench
    p, _ = bench.make_params(capi, synth, types.SimpleNamespace(yaml=None, config="cfg2", radius_cells=5.0, res=0.05))
    op = oracle.default_params()
    for f, _ in op._fields_:
        setattr(op, f, getattr(p, f))
    elev = synth.perlin_elevation(1024, 1024, seed=1234)
    g = oracle.geom(1024, 1024, 0.05)
    oracle.set_threads(min(os.cpu_count() or 1, 16))
    try:
        want = oracle.chain(g, op, elev)
        want["traversability_footprint"] = oracle.footprint(g, op, elev, want)
    finally:
        oracle.set_threads(1)
    for k in LAYERS:
        n_bad, mx, _ = compare_layer(k, got[k][0], want[k])
        assert n_bad == 0, (k, n_bad, mx)


def test_a_plain_run_of_the_headline_dumps_a_fixed_sample(tmp_path):
    """The 4096^2 headline's layers do not fit the dump's budget: a fixed sample of each, under 64 MB in all."""
    line = _bench("--steps", "5", "--warmup", "1", "--dump-outputs", str(tmp_path), full=False)
    assert line["config"]["name"] == "cfg3" and line["config"]["footprint"] is True and line["steps"] == 5
    arrays = [np.load(tmp_path / (k + ".npy")) for k in LAYERS]
    assert all(a.dtype == np.float32 and a.ndim == 1 and 0 < a.size < 4096 * 4096 and a.size == arrays[0].size for a in arrays)
    assert sum(os.path.getsize(tmp_path / (k + ".npy")) for k in LAYERS) <= 64 << 20
    assert all(np.isfinite(a).any() for a in arrays)
