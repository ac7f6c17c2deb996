"""params_yaml.window_expression_from_yaml: the SlidingWindowMathExpressionFilter entries of a filter chain file."""
import math

import pytest

from traversability_estimation_amd import params_yaml as P

STD_DEV = "sqrt(sumOfFinites(square(elevation - meanOfFinites(elevation))) ./ numberOfFinites(elevation))"
CHAIN = {"grid_map_filters": [
    {"name": "fill", "type": "gridMapFilters/MedianFillFilter", "params": {"input_layer": "elevation", "fill_hole_radius": 0.1}},
    {"name": "edges", "type": "gridMapFilters/SlidingWindowMathExpressionFilter",
     "params": {"input_layer": "elevation", "output_layer": "edges", "expression": STD_DEV, "compute_empty_cells": False, "edge_handling": "crop",
                "window_size": 5}},
    {"name": "box", "type": "gridMapFilters/SlidingWindowMathExpressionFilter",
     "params": {"input_layer": "elevation", "output_layer": "elevation_box", "expression": "meanOfFinites(elevation)", "window_length": 0.15}},
    {"name": "blur", "type": "gridMapFilters/MeanInRadiusFilter", "params": {"input_layer": "elevation", "output_layer": "smooth", "radius": 0.06}}]}


def test_entries_in_file_order():
    got = P.window_expression_from_yaml(CHAIN)
    assert got == [{"expression": STD_DEV, "input_layer": "elevation", "output_layer": "edges",
                    "params": {"window_size": 5, "compute_empty_cells": False, "edge_handling": "crop"}},
                   {"expression": "meanOfFinites(elevation)", "input_layer": "elevation", "output_layer": "elevation_box",
                    "params": {"window_length": 0.15, "compute_empty_cells": True, "edge_handling": "inside"}}]
    assert P.window_expression_from_yaml(CHAIN["grid_map_filters"]) == got  # a bare list of entries
    assert len(P.radius_filter_from_yaml(CHAIN)) == 1 and P.median_fill_from_yaml(CHAIN)["fill_hole_radius"] == 0.1  # (the others are still found)


def test_round_trip_through_a_file(tmp_path):
    yaml = pytest.importorskip("yaml")
    path = tmp_path / "chain.yaml"
    path.write_text(yaml.safe_dump(CHAIN))
    assert P.window_expression_from_yaml(str(path)) == P.window_expression_from_yaml(CHAIN)


def test_the_params_are_the_arguments_of_the_library(tmp_path):
    from traversability_estimation_amd import build, capi
    build.build_lib()
    for entry in P.window_expression_from_yaml(CHAIN):
        p = capi.window_expr_params(**entry["params"])
        assert (p.window_size, p.use_window_length) in ((5, 0), (0, 1))
        assert capi.window_expr_check(entry["expression"], entry["input_layer"])["layers"] == ["elevation"]


def test_a_file_without_them():
    assert P.window_expression_from_yaml({"traversability_map_filters": [{"type": "traversabilityFilters/StepFilter", "params": {}}]}) == []
    assert P.window_expression_from_yaml({}) == []


def test_refusals():
    def entry(**prm):
        return [{"type": "gridMapFilters/SlidingWindowMathExpressionFilter", "params": prm}]
    ok = {"input_layer": "a", "output_layer": "b", "expression": "mean(a)", "window_size": 3}
    assert P.window_expression_from_yaml(entry(**ok))[0]["params"]["window_size"] == 3
    with pytest.raises(P.ParamsYamlError, match="unknown parameter"):
        P.window_expression_from_yaml(entry(**ok, radius=0.1))
    for missing in ("input_layer", "output_layer", "expression"):
        with pytest.raises(P.ParamsYamlError, match=f"did not find param {missing}"):
            P.window_expression_from_yaml(entry(**{k: v for k, v in ok.items() if k != missing}))
    with pytest.raises(P.ParamsYamlError, match="exactly one of"):
        P.window_expression_from_yaml(entry(**ok, window_length=0.15))
    with pytest.raises(P.ParamsYamlError, match="exactly one of"):
        P.window_expression_from_yaml(entry(**{k: v for k, v in ok.items() if k != "window_size"}))
    for bad in (0, 2, -3, 3.0, True):
        with pytest.raises(P.ParamsYamlError, match="window_size must be an odd integer"):
            P.window_expression_from_yaml(entry(**dict(ok, window_size=bad)))
    base = {k: v for k, v in ok.items() if k != "window_size"}
    for bad in (-0.1, math.nan, math.inf):
        with pytest.raises(P.ParamsYamlError, match="window_length must be finite"):
            P.window_expression_from_yaml(entry(**base, window_length=bad))
    with pytest.raises(P.ParamsYamlError, match="edge_handling must be one of"):
        P.window_expression_from_yaml(entry(**ok, edge_handling="wrap"))
    with pytest.raises(P.ParamsYamlError, match="compute_empty_cells must be true or false"):
        P.window_expression_from_yaml(entry(**ok, compute_empty_cells="yes"))
    with pytest.raises(P.ParamsYamlError, match="the expression is empty"):
        P.window_expression_from_yaml(entry(**dict(ok, expression="  ")))
    # a refused entry stops the whole read: nothing is half-applied
    with pytest.raises(P.ParamsYamlError):
        P.window_expression_from_yaml(entry(**ok) + entry(**dict(ok, window_size=4)))
