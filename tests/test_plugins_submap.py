"""TraversabilityMap::getTraversabilityMap(position, length, layers, message) (plugins/test/plugin_submap_test.cpp): the body of
the reference's get_traversability service on the device -- the serialised submap parses, carries getSubmap's geometry and the
cells getTraversabilityMap() returns for the same rectangle; a request getSubmap refuses gives isSuccess = false."""
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
    exe = os.path.join(PLUG, "plugin_submap_test")
    src = os.path.join(PLUG, "test", "plugin_submap_test.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        runpy.run_path(os.path.join(PLUG, "build_plugins.py"))["build"]()
    return exe


@pytest.mark.gpu
def test_submap_service_body(driver):
    r = subprocess.run([driver], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK (0 failures)" in r.stdout
