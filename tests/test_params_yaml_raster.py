"""NormalVectorsFilter's `algorithm` key in the reference's filter file: area (the default) and raster are read, anything else
is refused; raster is an option of the context (TE_OPT_NORMALS_ALGORITHM), so the readers that return te_params alone refuse
it instead of describing the area method's chain."""
import os

import pytest
import yaml

from tests.conftest import ROOT
from traversability_estimation_amd import params_yaml as Y

GOLDEN = os.path.join(ROOT, "tests", "golden", "config", "robot_filter_parameter.yaml")


class FakeCapi:
    """default_params / validate_params without the library: the functions only pass values through."""
    RUN_KEEP_NORMALS = 1
    OPT_NORMALS_ALGORITHM = 13

    def default_params(self, **over):
        return dict(over)

    def validate_params(self, p):
        return p


def golden(algorithm=None, radius=True):
    """The reference's own file as a document, with `algorithm` added to / `radius` taken from the NormalVectorsFilter entry."""
    with open(GOLDEN) as f:
        doc = yaml.safe_load(f)
    nrm = doc[Y.CHAIN_KEY][0]
    assert nrm["type"] == "gridMapFilters/NormalVectorsFilter" and "algorithm" not in nrm["params"] and "radius" in nrm["params"]
    if algorithm is not None:
        nrm["params"]["algorithm"] = algorithm
    if not radius:
        del nrm["params"]["radius"]
    return doc


@pytest.mark.parametrize("radius", [True, False])
def test_raster_is_read_with_and_without_a_radius(radius):
    f = Y.filter_chain_fields(golden("raster", radius))
    assert f["normals_algorithm"] == 1
    assert ("normals_radius" in f) == radius  # absent: te_params_default's value stays
    plain = Y.filter_chain_fields(golden())
    assert {k: v for k, v in f.items() if k not in ("normals_algorithm", "normals_radius")} == \
        {k: v for k, v in plain.items() if k not in ("normals_algorithm", "normals_radius")}


def test_the_unchanged_file_and_an_explicit_area_give_0():
    assert Y.filter_chain_fields(golden())["normals_algorithm"] == 0
    assert Y.filter_chain_fields(golden("area"))["normals_algorithm"] == 0
    assert Y.filter_chain_fields(golden())["normals_radius"] == 0.05


def test_area_still_needs_its_radius():
    with pytest.raises(Y.ParamsYamlError, match="radius"):
        Y.filter_chain_fields(golden("area", radius=False))
    with pytest.raises(Y.ParamsYamlError, match="radius"):
        Y.filter_chain_fields(golden(None, radius=False))


@pytest.mark.parametrize("value", ["foo", "Raster", "", 1])
def test_any_other_algorithm_is_refused(value):
    with pytest.raises(Y.ParamsYamlError, match="algorithm"):
        Y.filter_chain_fields(golden(value))


def test_params_options_from_yaml_hands_the_option_over():
    capi = FakeCapi()
    text = yaml.safe_dump(golden("raster", radius=False)) + "\n"
    p, flags, options = Y.params_options_from_yaml(capi, text)
    assert options == {13: 1} and flags == 0 and "normals_algorithm" not in p and "normals_radius" not in p and "keep_normals" not in p
    p0, flags0, options0 = Y.params_options_from_yaml(capi, GOLDEN)
    assert options0 == {13: 0} and (p0, flags0) == Y.params_from_yaml(capi, GOLDEN)


def test_readers_without_a_place_for_the_option_refuse_raster():
    """params_from_yaml returns (te_params, flags): a raster file must not come back as the area method's parameters."""
    text = yaml.safe_dump(golden("raster")) + "\n"
    with pytest.raises(Y.ParamsYamlError, match="TE_OPT_NORMALS_ALGORITHM"):
        Y.params_from_yaml(FakeCapi(), text)
    with pytest.raises(Y.ParamsYamlError, match="TE_OPT_NORMALS_ALGORITHM"):
        Y.fields_from_yaml(text)
    assert "normals_algorithm" not in Y.fields_from_yaml(GOLDEN)
    assert Y.fields_from_yaml(text, normals_algorithm=True)["normals_algorithm"] == 1
