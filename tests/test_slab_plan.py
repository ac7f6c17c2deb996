"""The layout of a context's slab, planned by the library's OWN code: tests/cpu/slab_plan_check.cpp is compiled from
traversability_estimation_amd/csrc/te_slab.h, the header te_set_geometry allocates and assigns its pointers from.  Over the
named shapes (1x1x1, 100x133x1, 63x17x3, 64x16x1 and 65x17x1 either side of a flag tile, 4096^2, 32768^2, 512x512x4200) and
a seeded sweep, every part starts on a 256-byte boundary, the parts are in their order, contiguous and end at the total,
kSlabGuardRows rows of slack lie before the first layer and behind the last part -- the rows the marching kernels load
without a bounds check -- and every offset equals the expression te_set_geometry summed by hand before, restated in the
program (tests/test_gpu_fullsize.py sizes maps against device memory with the same total)."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpu", "slab_plan_check.cpp")
INC = os.path.join(ROOT, "traversability_estimation_amd", "csrc")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_slab_plan_over_named_and_random_shapes(tmp_path, flags):
    exe = str(tmp_path / "slab_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", INC, SRC, "-o", exe], check=True, timeout=300)
    for seed in (1, 2):
        r = subprocess.run([exe, "4000", str(seed)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
        assert "4016 shapes, 0 failed checks" in r.stdout
