"""The window mode of the expression compiler and the folds over a window (csrc/te_expr.h, csrc/te_window_plan.h) on the CPU:
tests/cpu/window_expr_check.cpp instantiates the evaluator and the folds the kernel of te_run_window_expression instantiates.
Its built-in checks run plain and -- as a stand-alone program -- under the sanitizers; its `eval` mode is compared with the numpy
restatement tests/ref_py/window_expression_ref.py on the bit patterns, on both folds."""
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.ref_py import expression_ref as E
from tests.ref_py import window_expression_ref as R

SRC = os.path.join(ROOT, "tests", "cpu", "window_expr_check.cpp")
INC = os.path.join(ROOT, "traversability_estimation_amd", "csrc")
STD_DEV = "sqrt(sumOfFinites(square(elevation - meanOfFinites(elevation))) ./ numberOfFinites(elevation))"


def build(tmp, flags):
    exe = str(tmp / "window_expr_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + flags + ["-I", INC, SRC, "-o", exe], check=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("window_expr"), ["-O2"])


def out(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout.strip()


def test_built_in_checks(exe):
    assert ", 0 failed checks" in out(exe)


def test_built_in_checks_under_the_sanitizers(tmp_path):
    assert ", 0 failed checks" in out(build(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


def test_the_standard_deviation_compiles_to_three_reductions_with_levels(exe):
    words = out(exe, "compile", STD_DEV, 0).split()
    assert words[0] == "OK" and words[2:4] == ["3", "1"] and words[5:] == ["1", "0", "0"], words
    assert out(exe, "compile", "meanOfFinites(elevation)", 0).split()[2:4] == ["1", "0"]


@pytest.mark.parametrize("text,layer,kind,column,word", [
    ("abs(elevation)", 0, "BAD_PARAM", 1, "scalar"),
    ("elevation - meanOfFinites(elevation)", 0, "BAD_PARAM", 1, "scalar"),
    ("sum(mean(sumOfFinites(elevation)))", 0, "BAD_PARAM", 10, "nest"),
    ("meanOfFinites(traversability)", 0, "BAD_PARAM", 15, "input layer"),
    ("sum(elevation) + sum(elevation) + sum(elevation) + sum(elevation) + sum(elevation)", 0, "BAD_PARAM", 69, "more than 4 reductions"),
    ("sum(elevation * elevation)", 0, "UNSUPPORTED", 15, "matrix product"),
    ("sum(transpose(elevation))", 0, "UNSUPPORTED", 5, "not built"),
])
def test_refusals_carry_class_and_column(exe, text, layer, kind, column, word):
    line = out(exe, "compile", text, layer)
    assert line.startswith(f"ERR {kind} expression, column {column}:") and word in line, line
    if "more than" in word:  # (the limits of the compiled form are the library's own: the restatement does not model them)
        return
    with pytest.raises(E.ExprError) as e:  # and the numpy restatement refuses it with the same class
        R.window_expression(np.zeros((3, 3), np.float32), text, "elevation", 3, "crop")
    assert e.value.kind == kind


def window_map(seed, rows, cols):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 3.0, (rows, cols)).astype(np.float32)
    a[rng.random((rows, cols)) < 0.15] = np.nan
    a[rng.random((rows, cols)) < 0.03] = np.inf
    a[rng.random((rows, cols)) < 0.05] *= np.float32(1.0e6)
    return a


TEXTS = [STD_DEV, "meanOfFinites(elevation)", "maxOfFinites(elevation) - minOfFinites(elevation)", "sum(elevation)", "mean(elevation)",
         "numberOfFinites(elevation)", "2.5 - 1", "2 * meanOfFinites(elevation) - minOfFinites(elevation)", "sumOfFinites(cwiseMax(0, elevation))",
         "mean(2)", "sum(abs(elevation - maxOfFinites(elevation)) ./ 3)"]


@pytest.mark.parametrize("edge", range(4))
def test_the_evaluator_matches_the_numpy_restatement_bit_for_bit(exe, tmp_path, edge):
    rows, cols = 11, 9
    a = window_map(edge, rows, cols)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    a.T.astype(np.float32).tofile(src)  # column-major
    for text in TEXTS:
        for w in (1, 3, 5, 13, 23):
            for empty in (1, 0):
                want = R.window_expression(a, text, "elevation", w, R.EDGES[edge], bool(empty))
                for route in (2, 1):
                    assert out(exe, "eval", text, 0, rows, cols, w, edge, empty, route, src, dst).startswith("OK")
                    got = np.fromfile(dst, np.float32).reshape(cols, rows).T
                    assert E.same_bits(got, want), (text, w, R.EDGES[edge], empty, route, got, want)
