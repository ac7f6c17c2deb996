"""Context.run_filter_chain on the device: the demo-style chain file fused and unfused, each of its layers against the numpy
references chained in file order, and the reference's own file through the runner against te_run_chain."""
import os

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.ref_py import expression_ref as E
from tests.ref_py import median_fill_ref, pointwise_ref, radius_filter_ref, window_expression_ref
from tests.ref_py.grid_map_ref import GridMapRef
from tests.test_gpu_plugin_filters import OUT_LAYERS, assert_layers_match  # the plugin route's comparison, not a copy of it
from tests.user_layer_cases import RES, SHAPES, context, grid, same

pytestmark = pytest.mark.gpu
CHAINS = os.path.join(ROOT, "tests", "golden", "config", "chains")
OUTPUTS = ("elevation_filled", "elevation_smooth", "edges", "relief", "relief_raw", "score")


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    return capi


@pytest.fixture(scope="module")
def demo():
    from traversability_estimation_amd import params_yaml
    return params_yaml.filter_chain_from_yaml(os.path.join(CHAINS, "demo_chain.yaml"))


def terrain(rows, cols, batch, seed):
    """[batch][cols][rows]: a smooth relief with a step and noise, 5 % NaN with a NaN border strip and a NaN block"""
    rng = np.random.default_rng(seed)
    i, j = np.arange(rows, dtype=np.float32)[None, None, :], np.arange(cols, dtype=np.float32)[None, :, None]
    a = (0.2 * np.sin(i / 7.0) * np.cos(j / 5.0) + 0.15 * (j > cols // 2) + 0.02 * rng.standard_normal((batch, cols, rows))).astype(np.float32)
    a[rng.random(a.shape) < 0.03] = np.nan
    a[:, :, 0] = np.nan
    a[:, cols // 3:cols // 3 + 8, rows // 2:rows // 2 + 9] = np.nan  # (wider than the fill reaches: holes survive)
    return a


_REF = {}


def reference(rows, cols, batch, seed):
    """the numpy references chained in file order; computed once, never changed.  Layers as [batch][cols][rows]."""
    key = (rows, cols, batch, seed)
    if key in _REF:
        return _REF[key]
    elev = terrain(rows, cols, batch, seed)
    gm = GridMapRef(rows, cols, RES, (0.0, 0.0))
    per_map = lambda fn, a: np.stack([fn(m.T).T for m in a]).astype(np.float32)  # the references take (rows, cols)
    L = {"elevation": elev}
    L["elevation_filled"] = per_map(lambda m: median_fill_ref.median_fill(m, RES, 0.11, False, 0.0, 1)[0], elev)
    L["elevation_smooth"] = per_map(lambda m: radius_filter_ref.radius_filter(m, gm, 0.11, radius_filter_ref.MEAN), L["elevation_filled"])
    L["elevation_min"] = per_map(lambda m: radius_filter_ref.radius_filter(m, gm, 0.11, radius_filter_ref.MIN), L["elevation_filled"])
    L["edges"] = per_map(lambda m: window_expression_ref.window_expression(m, "maxOfFinites(elevation) - minOfFinites(elevation)",
                                                                         "elevation", 3, "crop", True), L["elevation_smooth"])
    # (the expression reference knows the reference's layer names: the same texts over layers that hold the same values)
    L["relief_raw"] = E.evaluate("traversability_slope - traversability_step", {"traversability_slope": L["elevation_filled"], "traversability_step": L["elevation_min"]})
    score = E.evaluate("1 - (traversability_slope ./ 0.05 + traversability_step ./ 0.1) / 2", {"traversability_slope": L["edges"], "traversability_step": L["relief_raw"]})
    L["score"] = pointwise_ref.thresholds(score, [("lower", 0.25, 0.0), ("upper", 0.9, 1.0)])
    L["relief"] = pointwise_ref.threshold(L["relief_raw"], "upper", 0.05, 0.05)
    for v in L.values():
        v.setflags(write=False)
    _REF[key] = L
    return L


@pytest.mark.parametrize("rows, cols, batch", SHAPES)
def test_demo_chain_fused_unfused_and_against_numpy(capi, demo, rows, cols, batch):
    want = reference(rows, cols, batch, 11)
    got = {}
    for fuse in (True, False):
        with context(capi, rows, cols, batch) as ctx:
            ctx.upload_elevation(want["elevation"])
            calls = ctx.run_filter_chain(demo, fuse=fuse)
            got[fuse] = {k: grid(ctx, k) for k in OUTPUTS}
            names = [c[0] for c in calls]
            # the layers the file names were added, the one it deletes is gone, the others stay
            assert names.count("te_add_layer") == 7 and names[-1] == "te_remove_layer" and calls[-1][1] == ("elevation_min",)
            with pytest.raises(capi.TeError):
                ctx.layer_id("elevation_min")
            work = [n for n in names if n not in ("te_add_layer", "te_remove_layer")]
            if fuse:
                assert work == ["te_run_median_fill", "te_run_radius_filter", "te_run_radius_filter", "te_run_window_expression", "te_run_layer_expression",
                                "te_copy_layer", "te_run_layer_expression_thresholds", "te_run_threshold"]
                fused = [c for c in calls if c[0] == "te_run_layer_expression_thresholds"][0]
                assert fused[1][1:] == ("score", [("lower", 0.25, 0.0), ("upper", 0.9, 1.0)])
            else:
                assert work == ["te_run_median_fill", "te_run_radius_filter", "te_run_radius_filter", "te_run_window_expression", "te_run_layer_expression",
                                "te_copy_layer", "te_run_layer_expression", "te_run_threshold", "te_run_threshold", "te_run_threshold"]
    for k in OUTPUTS:
        assert same(got[True][k], got[False][k]), k      # fused equals the steps one by one
        assert same(got[True][k], want[k]), k            # ... and the numpy references chained in file order
    assert (got[True]["score"] == 0.0).any() and (got[True]["score"] == 1.0).any()  # (both thresholds took effect)
    assert (got[True]["relief"] == np.float32(0.05)).any() and not same(got[True]["relief"], got[True]["relief_raw"])


def test_reference_yaml_through_the_runner_equals_te_run_chain(capi):
    from traversability_estimation_amd import params_yaml
    path = os.path.join(CHAINS, "robot_filter_parameter.yaml")
    steps = params_yaml.filter_chain_from_yaml(path)
    rows, cols, batch = SHAPES[1]
    rng = np.random.default_rng(5)
    i, j = np.arange(rows, dtype=np.float32)[None, None, :], np.arange(cols, dtype=np.float32)[None, :, None]
    elev = (0.1 * np.sin(i / 9.0) + 0.08 * np.cos(j / 6.0) + 0.01 * rng.standard_normal((batch, cols, rows))).astype(np.float32)
    elev[rng.random(elev.shape) < 0.05] = np.nan
    p, flags = params_yaml.params_from_yaml(capi, path)
    with capi.Context(0) as A, capi.Context(0) as B:
        for ctx in (A, B):
            ctx.set_geometry(rows, cols, batch, RES)
        A.set_params(p)
        A.upload_elevation(elev)
        A.run_chain(flags)
        B.set_params(capi.default_params(normals_radius=0.2, slope_critical=0.3, step_critical=0.5, rough_critical=0.4, w_scale=1.0))  # the file must win
        B.upload_elevation(elev)
        calls = B.run_filter_chain(steps)
        assert [c for c in calls if c[0] == "te_run_filter"] == [("te_run_filter", (f,)) for f in ("normals", "slope", "step", "roughness", "combine")]
        assert not [c for c in calls if c[0] in ("te_add_layer", "te_remove_layer", "te_run_layer_expression")]
        want = {k: A.download(k) for k in OUT_LAYERS + ("elevation",)}
        got = {k: B.download(k) for k in OUT_LAYERS + ("elevation",)}
    assert_layers_match(got, want, ctx="robot_filter_parameter.yaml through run_filter_chain")
    assert same(got["elevation"], want["elevation"])
    for k in OUT_LAYERS:
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
