"""tests/cpu/expr_fuzz.cpp: the compiler of csrc/te_expr.h under 200 000 seeded texts (valid, mutated, truncated, random bytes,
nesting 10 000 deep), as a stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer and run directly on
the host (nothing is loaded into Python)."""
import os
import re
import subprocess

from tests.conftest import ROOT


def test_the_expression_compiler_survives_the_fuzzer_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "expr_fuzz")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "traversability_estimation_amd", "csrc"), os.path.join(ROOT, "tests", "cpu", "expr_fuzz.cpp"), "-o", exe],
                   check=True, timeout=300)
    r = subprocess.run([exe, "200000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    m = re.fullmatch(r"ok compiled=(\d+) rejected=(\d+) unsupported=(\d+)\n", r.stdout)
    assert m, r.stdout
    ok, bad, unsupported = (int(v) for v in m.groups())
    assert ok + bad + unsupported == 200008  # (+ the eight deep texts)
    # every verdict occurs often: the texts reach past the first token
    assert ok > 20000 and bad > 20000 and unsupported > 2000, m.groups()
