"""params_yaml.filter_chain_from_yaml and plan_filter_chain on the fixtures under tests/golden/config/chains/: the steps a
chain file gives, which thresholds ride in an expression's launch, and every refusal with the entry's name."""
import os

import pytest

from tests.conftest import ROOT
from traversability_estimation_amd import params_yaml as Y

CHAINS = os.path.join(ROOT, "tests", "golden", "config", "chains")


def steps_of(name, key=None):
    return Y.filter_chain_from_yaml(os.path.join(CHAINS, name), key)


def test_demo_chain_steps():
    s = steps_of("demo_chain.yaml")
    assert [(x["name"], x["filter"]) for x in s] == [
        ("fill", "median_fill"), ("smooth", "radius"), ("lowest", "radius"), ("edges", "window_expression"), ("relief", "expression"),
        ("keep_relief", "duplication"), ("score", "expression"), ("score_lower", "threshold"), ("score_upper", "threshold"),
        ("relief_cap", "threshold"), ("drop", "deletion")]
    assert s[0] == {"name": "fill", "filter": "median_fill", "input_layer": "elevation", "output_layer": "elevation_filled",
                    "params": {"fill_hole_radius": 0.11, "filter_existing_values": 0, "existing_value_radius": 0.0, "num_erode_dilation_iterations": 1}}
    assert s[1] == {"name": "smooth", "filter": "radius", "op": "mean", "radius": 0.11, "input_layer": "elevation_filled", "output_layer": "elevation_smooth"}
    assert s[2]["op"] == "min" and s[2]["output_layer"] == "elevation_min"
    assert s[3] == {"name": "edges", "filter": "window_expression", "input_layer": "elevation_smooth", "output_layer": "edges",
                    "expression": "maxOfFinites(elevation_smooth) - minOfFinites(elevation_smooth)",
                    "params": {"window_size": 3, "compute_empty_cells": True, "edge_handling": "crop"}}
    assert s[4] == {"name": "relief", "filter": "expression", "expression": "elevation_filled - elevation_min", "output_layer": "relief"}
    assert s[5] == {"name": "keep_relief", "filter": "duplication", "input_layer": "relief", "output_layer": "relief_raw"}
    assert s[7] == {"name": "score_lower", "filter": "threshold", "layer": "score", "mode": "lower", "threshold": 0.25, "set_to": 0.0}
    assert s[8] == {"name": "score_upper", "filter": "threshold", "layer": "score", "mode": "upper", "threshold": 0.9, "set_to": 1.0}
    assert s[10] == {"name": "drop", "filter": "deletion", "layers": ["elevation_min"]}
    # the same list under its key, and a key the file does not have
    assert steps_of("demo_chain.yaml", "grid_map_filters") == s
    with pytest.raises(Y.ParamsYamlError, match="no filter list named 'other'"):
        steps_of("demo_chain.yaml", "other")


def test_reference_chain_steps_and_the_file_is_the_reference_s():
    with open(os.path.join(CHAINS, "robot_filter_parameter.yaml"), "rb") as a, open(os.path.join(ROOT, "tests", "golden", "config", "robot_filter_parameter.yaml"), "rb") as b:
        assert a.read() == b.read()
    s = steps_of("robot_filter_parameter.yaml")
    assert [x["filter"] for x in s] == ["normals", "slope", "step", "roughness", "expression", "deletion"]
    assert s[0]["fields"] == {"normals_radius": 0.05, "normals_axis": 2} and s[0]["algorithm"] == "area"
    assert s[1]["fields"] == {"slope_critical": 1.0}
    assert s[2]["fields"] == {"step_critical": 0.12, "step_radius1": 0.04, "step_radius2": 0.04, "step_ncrit": 4, "fp_critical_step": 0.12}
    assert s[3]["fields"] == {"rough_critical": 0.05, "rough_radius": 0.05}
    assert s[4]["output_layer"] == "traversability" and Y.parse_weighted_sum(s[4]["expression"])["w_slope"] == 1.0
    assert s[5]["layers"] == ["surface_normal_x", "surface_normal_y", "surface_normal_z"]
    # the existing reader of the fixed chain reads the same values from the same file
    f = Y.fields_from_yaml(os.path.join(CHAINS, "robot_filter_parameter.yaml"))
    for x in s[:4]:
        for k, v in x["fields"].items():
            assert f[k] == v, k


def names(plan):
    return [(kind, s["name"], None if fused is None else [t["name"] for t in fused]) for kind, s, fused in plan]


def test_fusion_decisions():
    demo = names(Y.plan_filter_chain(steps_of("demo_chain.yaml")))
    assert ("expression", "relief", []) in demo                       # the duplication follows: nothing to fuse
    assert ("expression", "score", ["score_lower", "score_upper"]) in demo
    assert ("threshold", "relief_cap", None) in demo                   # another layer, behind other filters
    assert [n for _, n, _ in demo if n.startswith("score_")] == []     # the fused thresholds are no calls of their own
    s = steps_of("fusion_cases.yaml")
    assert names(Y.plan_filter_chain(s)) == [
        ("expression", "a", []), ("duplication", "copy", None), ("threshold", "a_late", None),   # a filter in between
        ("expression", "c", ["c1", "c2", "c3", "c4"]), ("threshold", "c5", None), ("threshold", "c6", None),  # n > 4 is split
        ("expression", "d", []), ("threshold", "other", None)]                                    # a threshold on another layer
    unfused = names(Y.plan_filter_chain(s, fuse=False))
    assert [k for k, _, _ in unfused] == [x["filter"] for x in s] and all(f in (None, []) for _, _, f in unfused)


REFUSALS = {
    "unknown_type": "filter 'curve': type 'gridMapFilters/CurvatureFilter' is not built",
    "threshold_both": "filter 'clamp': ThresholdFilter: exactly one of lower_threshold and upper_threshold (got both)",
    "threshold_neither": "filter 'clamp': ThresholdFilter: exactly one of lower_threshold and upper_threshold (got neither)",
    "threshold_two_layers": "filter 'clamp': ThresholdFilter: the filter runs in place",
    "unknown_key": "filter 'dup': DuplicationFilter: unknown parameter(s) ['radius']",
    "missing_key": "filter 'expr': MathExpressionFilter did not find param expression",
    "window_even": "filter 'win': SlidingWindowMathExpressionFilter: window_size must be an odd integer",
    "radius_negative": "filter 'near': MinInRadiusFilter: radius must be finite and not negative",
    "deletion_reference": "filter 'drop': DeletionFilter: ['traversability_slope'] are layers of the context itself",
    "normals_input": "filter 'normals': NormalVectorsFilter: input_layer must be 'elevation'",
    "map_type": "filter 'slope': SlopeFilter: map_type must stay 'traversability_slope'",
}


def test_every_refusal_fixture_has_a_case():
    assert sorted(f[len("refused_"):-len(".yaml")] for f in os.listdir(CHAINS) if f.startswith("refused_")) == sorted(REFUSALS)


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusal_names_the_entry(case):
    with pytest.raises(Y.ParamsYamlError) as e:
        steps_of("refused_%s.yaml" % case)
    assert REFUSALS[case] in str(e.value), str(e.value)


def test_existing_readers_keep_refusing():
    """The fixed chain's reader still refuses a chain file it cannot honour."""
    with pytest.raises(Y.ParamsYamlError):
        Y.fields_from_yaml(os.path.join(CHAINS, "demo_chain.yaml"))
