"""tests/cpu/out_msg_check.cpp: the parsers of the two output messages (te_occupancy.h, te_cloud.h) on corrupted inputs, as a
stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer and run directly (nothing is loaded into
Python)."""
import os
import re
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("out_msg") / "out_msg_check"
    src = os.path.join(ROOT, "tests", "cpu", "out_msg_check.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "traversability_estimation_amd", "csrc"), src, "-o", str(out)],
                   check=True, timeout=300)
    return str(out)


def test_parsers_survive_corrupted_input_under_the_sanitizers(exe):
    r = subprocess.run([exe, "40000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    m = re.fullmatch(r"ok occupancy=(\d+)/(\d+) cloud=(\d+)/(\d+)\n", r.stdout)
    assert m, r.stdout
    o_ok, o_bad, c_ok, c_bad = (int(v) for v in m.groups())
    assert o_ok + o_bad == c_ok + c_bad == 40000
    # both verdicts occur often: the mutations reach the checks and the payload alike
    assert o_ok > 2000 and o_bad > 10000 and c_ok > 2000 and c_bad > 10000, m.groups()
