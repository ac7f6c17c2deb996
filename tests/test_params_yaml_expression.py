"""params_yaml.chain_expression / params_and_expression_from_yaml: a filter file whose MathExpressionFilter is not the weighted
sum is no longer a dead end -- the text comes back for te_run_expression -- while params_from_yaml keeps refusing it."""
import os

import pytest

from tests.conftest import ROOT
from traversability_estimation_amd import params_yaml as Y

CFG = os.path.join(ROOT, "tests", "golden", "config")
SHIPPED = "(1.0 / 3.0) * (traversability_slope + traversability_step + traversability_roughness)"
MIN3 = "cwiseMin(cwiseMin(traversability_slope, traversability_step), traversability_roughness)"


class FakeCapi:
    """default_params / validate_params / expr_check without the library: the functions only pass values through."""
    RUN_KEEP_NORMALS = 1

    def __init__(self):
        self.checked = []

    def default_params(self, **over):
        return dict(over)

    def validate_params(self, p):
        return p

    def expr_check(self, text):
        self.checked.append(text)


def min_file():
    with open(os.path.join(CFG, "robot_filter_parameter.yaml")) as f:
        text = f.read()
    assert SHIPPED in text
    return text.replace(SHIPPED, MIN3)


def test_the_reference_file_is_a_weighted_sum():
    assert Y.chain_expression(os.path.join(CFG, "robot_filter_parameter.yaml")) == (SHIPPED, True)
    capi = FakeCapi()
    p, flags, text = Y.params_and_expression_from_yaml(capi, os.path.join(CFG, "robot_filter_parameter.yaml"))
    assert text is None and flags == 0 and p["w_scale"] == pytest.approx(1.0 / 3.0, rel=1e-7) and not capi.checked
    assert (p, flags) == Y.params_from_yaml(capi, os.path.join(CFG, "robot_filter_parameter.yaml"))


def test_a_min_style_file_yields_its_text_and_default_weights():
    doc = min_file()
    assert Y.chain_expression(doc) == (MIN3, False)
    capi = FakeCapi()
    p, flags, text = Y.params_and_expression_from_yaml(capi, doc, os.path.join(CFG, "robot_footprint_parameter.yaml"), os.path.join(CFG, "robot.yaml"))
    assert text == MIN3 and capi.checked == [MIN3] and flags == 0
    assert not any(k.startswith("w_") for k in p)  # the weights stay at the library's defaults
    ref = Y.fields_from_yaml(os.path.join(CFG, "robot_filter_parameter.yaml"), os.path.join(CFG, "robot_footprint_parameter.yaml"), os.path.join(CFG, "robot.yaml"))
    ref.pop("keep_normals")
    assert p == {k: v for k, v in ref.items() if not k.startswith("w_")}  # every other field as the weighted-sum file gives it


def test_params_from_yaml_still_refuses_it():
    with pytest.raises(Y.ParamsYamlError, match="weighted sum"):
        Y.params_from_yaml(FakeCapi(), min_file())
    with pytest.raises(Y.ParamsYamlError, match="weighted sum"):
        Y.parse_weighted_sum(MIN3)
    with pytest.raises(Y.ParamsYamlError, match="weighted sum"):
        Y.fields_from_yaml(min_file())
