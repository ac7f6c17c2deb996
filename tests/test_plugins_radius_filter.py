"""traversabilityFilters/MeanInRadiusFilter, MinInRadiusFilter and TraversabilityMap::setSmoothElevation
(plugins/test/plugin_radius_filter_test.cpp): the adapters compile against the stub ROS headers, configure() takes the upstream filters'
keys and refuses a bad radius, and update() returns the layer filtered on the device, bit for bit the contract restated in the driver."""
import os
import re
import subprocess

import pytest

from tests.conftest import ROOT

PLUG = os.path.join(ROOT, "traversability_estimation_amd", "plugins")


@pytest.fixture(scope="module")
def driver():
    import runpy
    from oracle import oracle as O
    from traversability_estimation_amd import build
    build.build_lib()
    O.build()
    exe = os.path.join(PLUG, "plugin_radius_filter_test")
    src = os.path.join(PLUG, "test", "plugin_radius_filter_test.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        runpy.run_path(os.path.join(PLUG, "build_plugins.py"))["build"]()
    return exe


def test_the_adapters_build_and_are_exported(driver):
    assert os.path.exists(driver)
    xml = open(os.path.join(PLUG, "filter_plugins.xml")).read()
    names = re.findall(r'<class name="([^"]+)"', xml)
    assert "traversabilityFilters/MeanInRadiusFilter" in names and "traversabilityFilters/MinInRadiusFilter" in names
    # the three reference entries and the earlier additions are where they were
    assert names[:5] == ["traversabilityFilters/SlopeFilter", "traversabilityFilters/StepFilter", "traversabilityFilters/RoughnessFilter",
                         "traversabilityFilters/SurfaceNormalsFilter", "traversabilityFilters/MedianFillFilter"]
    cmake = open(os.path.join(PLUG, "CMakeLists.txt")).read()
    assert "src/MeanInRadiusFilter.cpp" in cmake and "src/MinInRadiusFilter.cpp" in cmake


@pytest.mark.gpu
def test_radius_filter_plugins(driver):
    r = subprocess.run([driver], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK (0 failures)" in r.stdout
