"""The C++ Step and Roughness plugin adapters at radii above 32 cells (0.40 m windows, a 0.41 m estimation radius on a
0.01 m map): the plugins set TE_OPT_FILTER_ANY_RADIUS = 1 on their context, so update() returns true and matches the
oracle (plugins/test/plugin_radius_test.cpp)."""
import os
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
    exe = os.path.join(PLUG, "plugin_radius_test")
    src = os.path.join(PLUG, "test", "plugin_radius_test.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        runpy.run_path(os.path.join(PLUG, "build_plugins.py"))["build"]()
    return exe


@pytest.mark.gpu
def test_step_and_roughness_plugins_at_40_cells(driver):
    r = subprocess.run([driver], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK (0 failures)" in r.stdout
