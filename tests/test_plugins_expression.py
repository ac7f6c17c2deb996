"""FusedChainFilter with the optional `expression` parameter (plugins/test/plugin_expression_test.cpp): the chain, then the
expression on the device, equal the oracle chain's scores folded with the same expression; configure() refuses a text the
library refuses."""
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
    exe = os.path.join(PLUG, "plugin_expression_test")
    src = os.path.join(PLUG, "test", "plugin_expression_test.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        runpy.run_path(os.path.join(PLUG, "build_plugins.py"))["build"]()
    return exe


@pytest.mark.gpu
def test_fused_chain_with_an_expression(driver):
    r = subprocess.run([driver], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK (0 failures)" in r.stdout
