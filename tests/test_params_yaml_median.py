"""params_yaml.median_fill_from_yaml: the settings of a gridMapFilters/MedianFillFilter entry, and that the functions that read
the chain keep refusing what they refused (no GPU, no library)."""
import os

import pytest

from tests.conftest import ROOT
from traversability_estimation_amd import params_yaml as Y

SHIPPED = os.path.join(ROOT, "tests", "golden", "config", "robot_filter_parameter.yaml")

FILL = """
traversability_map_filters:
  - name: fill
    type: gridMapFilters/MedianFillFilter
    params:
      input_layer: elevation
      output_layer: elevation_inpainted
      fill_hole_radius: 0.15
      filter_existing_values: true
      existing_value_radius: 0.11
      num_erode_dilation_iterations: 2
      fill_mask_layer: fill_mask
      debug: false
  - name: other
    type: gridMapFilters/DeletionFilter
    params:
      layers: [x]
"""


def test_the_shipped_file_has_no_fill():
    assert Y.median_fill_from_yaml(SHIPPED) is None
    assert Y.median_fill_from_yaml({"traversability_map_filters": []}) is None
    assert Y.median_fill_from_yaml({}) is None


def test_every_key_is_read():
    got = Y.median_fill_from_yaml(FILL)
    assert got == {"input_layer": "elevation", "output_layer": "elevation_inpainted", "fill_hole_radius": 0.15, "filter_existing_values": 1,
                   "existing_value_radius": 0.11, "num_erode_dilation_iterations": 2}
    cells = Y.median_fill_from_yaml(FILL, resolution=0.05)
    assert cells["fill_hole_cells"] == 2 and cells["existing_value_cells"] == 2  # 0.15 / 0.05 truncates to 2
    assert Y.median_fill_from_yaml(FILL, resolution=0.03)["existing_value_cells"] == 3


def test_defaults_and_a_bare_list():
    got = Y.median_fill_from_yaml([{"name": "f", "type": "gridMapFilters/MedianFillFilter", "params": {"input_layer": "elevation"}}])
    assert got == {"input_layer": "elevation", "output_layer": "elevation", "fill_hole_radius": 0.05, "filter_existing_values": 0,
                   "existing_value_radius": 0.0, "num_erode_dilation_iterations": 4}


@pytest.mark.parametrize("params,msg", [({"input_layer": "elevation", "radius": 0.1}, "unknown parameter"),
                                        ({"fill_hole_radius": 0.1}, "input_layer"),
                                        ({"input_layer": "elevation", "fill_hole_radius": -0.1}, "fill_hole_radius"),
                                        ({"input_layer": "elevation", "existing_value_radius": float("inf")}, "existing_value_radius"),
                                        ({"input_layer": "elevation", "num_erode_dilation_iterations": -1}, "num_erode_dilation_iterations")])
def test_refusals(params, msg):
    with pytest.raises(Y.ParamsYamlError, match=msg):
        Y.median_fill_from_yaml({"filters": [{"type": "gridMapFilters/MedianFillFilter", "params": params}]})


def test_two_entries_and_a_bad_resolution_are_refused():
    e = {"type": "gridMapFilters/MedianFillFilter", "params": {"input_layer": "elevation"}}
    with pytest.raises(Y.ParamsYamlError, match="2 MedianFillFilter"):
        Y.median_fill_from_yaml({"a": [e], "b": [e]})
    with pytest.raises(Y.ParamsYamlError, match="resolution"):
        Y.median_fill_from_yaml([e], resolution=0.0)


def test_the_chain_readers_still_refuse_a_chain_that_starts_with_the_fill():
    with pytest.raises(Y.ParamsYamlError, match="the filter chain must be"):
        Y.fields_from_yaml(FILL)
    assert "normals_radius" in Y.fields_from_yaml(SHIPPED)
