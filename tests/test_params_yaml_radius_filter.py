"""params_yaml.radius_filter_from_yaml: the MeanInRadiusFilter / MinInRadiusFilter entries of a filter chain file."""
import math

import pytest

from traversability_estimation_amd import params_yaml as P

CHAIN = {"grid_map_filters": [
    {"name": "fill", "type": "gridMapFilters/MedianFillFilter", "params": {"input_layer": "elevation", "fill_hole_radius": 0.1}},
    {"name": "blur", "type": "gridMapFilters/MeanInRadiusFilter", "params": {"input_layer": "elevation", "output_layer": "elevation_smooth", "radius": 0.06}},
    {"name": "low", "type": "gridMapFilters/MinInRadiusFilter", "params": {"input_layer": "elevation_smooth", "output_layer": "lower", "radius": 0.15}},
    {"name": "normals", "type": "gridMapFilters/NormalVectorsFilter", "params": {"input_layer": "elevation_smooth", "radius": 0.05}}]}


def test_entries_in_file_order():
    got = P.radius_filter_from_yaml(CHAIN)
    assert got == [{"op": "mean", "radius": 0.06, "input_layer": "elevation", "output_layer": "elevation_smooth"},
                   {"op": "min", "radius": 0.15, "input_layer": "elevation_smooth", "output_layer": "lower"}]
    assert P.radius_filter_from_yaml(CHAIN["grid_map_filters"]) == got  # a bare list of entries
    assert P.median_fill_from_yaml(CHAIN)["fill_hole_radius"] == 0.1    # (the fill beside them is still found)


def test_a_file_without_them():
    assert P.radius_filter_from_yaml({"traversability_map_filters": [{"type": "traversabilityFilters/StepFilter", "params": {}}]}) == []
    assert P.radius_filter_from_yaml({}) == []


def test_from_a_file(tmp_path):
    yaml = pytest.importorskip("yaml")
    path = tmp_path / "chain.yaml"
    path.write_text(yaml.safe_dump(CHAIN))
    assert len(P.radius_filter_from_yaml(str(path))) == 2


@pytest.mark.parametrize("kind", ["MeanInRadiusFilter", "MinInRadiusFilter"])
def test_refusals(kind):
    def entry(**prm):
        return [{"type": "gridMapFilters/" + kind, "params": prm}]
    ok = {"input_layer": "a", "output_layer": "b", "radius": 0.0}
    assert P.radius_filter_from_yaml(entry(**ok))[0]["radius"] == 0.0  # radius 0: the centre cell alone
    with pytest.raises(P.ParamsYamlError, match="unknown parameter"):
        P.radius_filter_from_yaml(entry(**ok, window_size=3))
    for missing in ok:
        with pytest.raises(P.ParamsYamlError, match=f"{kind} did not find param {missing}"):
            P.radius_filter_from_yaml(entry(**{k: v for k, v in ok.items() if k != missing}))
    for bad in (-0.1, math.nan, math.inf):
        with pytest.raises(P.ParamsYamlError, match="radius must be finite"):
            P.radius_filter_from_yaml(entry(**dict(ok, radius=bad)))
