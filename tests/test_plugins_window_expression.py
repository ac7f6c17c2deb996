"""traversabilityFilters/SlidingWindowMathExpressionFilter (plugins/test/plugin_window_expression_test.cpp): the adapter compiles
against the stub ROS headers, is listed, configure() takes the upstream filter's keys and refuses what it cannot honour, and
update() returns the expression over the windows computed on the device, bit for bit the contract restated in the driver."""
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
    exe = os.path.join(PLUG, "plugin_window_expression_test")
    src = os.path.join(PLUG, "test", "plugin_window_expression_test.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        runpy.run_path(os.path.join(PLUG, "build_plugins.py"))["build"]()
    return exe


def test_the_adapter_builds_and_is_listed(driver):
    assert os.path.exists(driver)
    xml = open(os.path.join(PLUG, "filter_plugins.xml")).read()
    names = re.findall(r'<class name="([^"]+)"', xml)
    assert "traversabilityFilters/SlidingWindowMathExpressionFilter" in names
    assert 'type="filters::SlidingWindowMathExpressionFilter<grid_map::GridMap>"' in xml
    # the three reference entries and the earlier additions are where they were
    assert names[:7] == ["traversabilityFilters/SlopeFilter", "traversabilityFilters/StepFilter", "traversabilityFilters/RoughnessFilter",
                         "traversabilityFilters/SurfaceNormalsFilter", "traversabilityFilters/MedianFillFilter",
                         "traversabilityFilters/MeanInRadiusFilter", "traversabilityFilters/MinInRadiusFilter"]
    assert "src/SlidingWindowMathExpressionFilter.cpp" in open(os.path.join(PLUG, "CMakeLists.txt")).read()
    assert "src/SlidingWindowMathExpressionFilter.cpp" in open(os.path.join(PLUG, "build_plugins.py")).read()


@pytest.mark.gpu
def test_window_expression_plugin(driver):
    r = subprocess.run([driver], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK (0 failures)" in r.stdout
