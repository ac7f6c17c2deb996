"""csrc/te_expr.h on the CPU (tests/cpu/expr_check.cpp, g++ -ffp-contract=off): the compiler's error classes, and the evaluator
the kernels instantiate against the independent numpy evaluator tests/ref_py/expression_ref.py, bit for bit (NaN payloads
apart).  The one reference-held pin: the shipped expression gives the bag's traversability layer from its three scores."""
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.ref_py import expression_ref as R

SHIPPED = "(1.0 / 3.0) * (traversability_slope + traversability_step + traversability_roughness)"
A, B, C = "traversability_slope", "traversability_step", "traversability_roughness"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("expr") / "expr_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "traversability_estimation_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpu", "expr_check.cpp"), "-o", str(out)], check=True, timeout=300)
    return str(out)


def status(exe, text):
    r = subprocess.run([exe, text], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return r.stdout.strip().split(" ", 2)


def run(exe, text, layers, tmp_path):
    """layers: name -> [maps, cells] float32; missing layers are NaN."""
    maps, cells = next(iter(layers.values())).shape
    full = np.full((15, maps, cells), np.nan, dtype=np.float32)
    for k, v in layers.items():
        full[R.LAYER_NAMES.index(k)] = v
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    full.tofile(fin)
    r = subprocess.run([exe, text, str(cells), str(maps), str(fin), str(fout)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("OK "), (text, r.stdout, r.stderr)
    return np.fromfile(fout, dtype=np.float32).reshape(maps, cells)


def layers_with_specials(seed, maps=2, cells=257):
    """Random values; NaN, +inf and -inf in every operand position against every other class of value."""
    rng = np.random.default_rng(seed)
    out = {}
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -2.5], dtype=np.float32)
    grid = np.stack(np.meshgrid(special, special, special, indexing="ij")).reshape(3, -1)  # 343 combinations
    for k, name in enumerate((A, B, C)):
        v = rng.uniform(-2.0, 2.0, size=(maps, cells)).astype(np.float32)
        v[0, :] = np.resize(grid[k], cells)
        out[name] = v
    out["elevation"] = rng.uniform(-1.0, 3.0, size=(maps, cells)).astype(np.float32)
    return out


ARITHMETIC = [
    f"{A}-{B}-{C}", f"{A}/{B}/{C}", f"2*-{A}", f"(1.0 / 3.0) * ({A} + {B} + {C})", SHIPPED,
    f"{A} + {B} * 2 - {C} / 4", f"{A} .* {B} ./ {C}", f"{A} / {B}", f"-({A} + {B}) .* -{C}", f"2.*{A} - .5*{B} + 1e-3*{C} - 3.",
    f"- - {A} + + {B}", f"({A} - 0.25) * (1.0 / 3.0 + 2) - 7 / 2 / 2", f"1 - 2 - 3 + {A}*0",
    f"abs({A} - {B})", f"sqrt({A})", f"square({A} + {B})", f"sqrt(abs({A})) .* square({C})",
    f"cwiseMin({A}, {B})", f"cwiseMax({A}, {B})", f"cwiseMin({B}, {A})", f"cwiseMax({B}, {A})", f"cwiseMax({A} - 0.5, 0.0)", f"cwiseMin(1.0, {A})",
    f"cwiseMin(cwiseMin({A}, {B}), {C})", f"cwiseMax(cwiseMin({A}, 1.0), 0.0) - cwiseMax(0.0, {B})",
]


@pytest.mark.parametrize("text", ARITHMETIC)
def test_arithmetic_and_elementwise_functions_match_the_reference_bit_for_bit(exe, tmp_path, text):
    layers = layers_with_specials(1)
    got = run(exe, text, layers, tmp_path)
    want = R.evaluate(text, layers)
    assert R.same_bits(got, want), (text, np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:5])


POWERS = [f"-{A}^2", f"(-{A})^2", f"2 ^ -1 * {A}", f"{A}^2^2", f"{A} .^ {B}", f"{B}^0.5 - {A}^2", f"2 .^ -{B}"]


@pytest.mark.parametrize("text", POWERS)
def test_powers_bind_as_in_matlab(exe, tmp_path, text):
    """^ is the C library's powf here and the float64 power in the reference: they agree bit for bit wherever the exact result
    is a float32, so the operands are small multiples of 1/8 (and the special values) -- the grouping is what this pins."""
    layers = layers_with_specials(3)
    rng = np.random.default_rng(4)
    layers[A][1] = rng.integers(-24, 25, size=layers[A].shape[1]) / 8.0
    layers[B][:] = rng.integers(0, 4, size=layers[B].shape)
    layers[B][0, :7] = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, 2.0]
    if "0.5" in text:
        layers[B][:] = np.square(rng.integers(0, 9, size=layers[B].shape) / 4.0)
    got = run(exe, text, layers, tmp_path)
    assert R.same_bits(got, R.evaluate(text, layers)), text


REDUCTIONS = [
    "elevation - meanOfFinites(elevation)", "(elevation - minOfFinites(elevation)) / (maxOfFinites(elevation) - minOfFinites(elevation))",
    "numberOfFinites(elevation) + 0 * elevation", "sumOfFinites(elevation) - elevation", f"maxOfFinites({A} .* {B}) - minOfFinites(abs({C}))",
    "numberOfFinites(elevation) / 2", "sum(elevation) + mean(elevation)", f"mean(abs({A})) * {A}",
]


@pytest.mark.parametrize("text", REDUCTIONS)
def test_reductions_per_map_match_the_reference_bit_for_bit(exe, tmp_path, text):
    # values on a 1/1024 grid: every partial sum is exact in double, so the order of the additions cannot show
    rng = np.random.default_rng(2)
    layers = {k: (rng.integers(-4096, 4096, size=(3, 331)) / 1024.0).astype(np.float32) for k in ("elevation", A, B, C)}
    for v in layers.values():
        v[0, rng.random(331) < 0.1] = np.nan
        v[0, rng.random(331) < 0.02] = np.inf
        v[0, rng.random(331) < 0.02] = -np.inf
        v[2, :] = np.nan  # a map without a finite cell (map 1 has no invalid cell at all)
    got = run(exe, text, layers, tmp_path)
    want = R.evaluate(text, layers)
    assert R.same_bits(got, want), text


def test_a_map_without_a_finite_cell(exe, tmp_path):
    layers = {"elevation": np.full((1, 5), np.nan, dtype=np.float32)}
    for name, want in (("minOfFinites", np.nan), ("maxOfFinites", np.nan), ("meanOfFinites", np.nan), ("sumOfFinites", 0.0), ("numberOfFinites", 0.0)):
        got = run(exe, f"{name}(elevation)", layers, tmp_path)
        assert R.same_bits(got, np.full((1, 5), want, dtype=np.float32)), name


def chain(n):
    """`n` additions of one layer nested to the right: n + 1 pushes, n additions, a stack of n + 1."""
    return "elevation" + " + (elevation" * n + ")" * n


ERRORS = [
    (f"{A} * {B}", "UNSUPPORTED", ".*"),
    ("traversability_slop + 1", "BAD_PARAM", "column 1"),
    ("elevation" + " + elevation" * 32, "BAD_PARAM", "64 instructions"),        # 33 pushes + 32 additions = 65
    (" + ".join(R.LAYER_NAMES[:9]), "BAD_PARAM", "8 distinct layers"),
    (chain(8), "BAD_PARAM", "deeper than 8"),                                     # nine operands on the stack
    (" + ".join(f"sum({n})" for n in R.LAYER_NAMES[:5]), "BAD_PARAM", "4 reductions"),
    ("sum(elevation - mean(elevation))", "BAD_PARAM", "do not nest"),
    ("(elevation + 1", "BAD_PARAM", "unbalanced"),
    ("elevation + 1)", "BAD_PARAM", "unbalanced"),
    ("", "BAD_PARAM", "empty"),
    ("   ", "BAD_PARAM", "empty"),
    ("elevation +", "BAD_PARAM", "column 12"),
    ("cwiseMin(elevation)", "BAD_PARAM", "two arguments"),
    ("abs(elevation, 1)", "BAD_PARAM", "one argument"),
    ("abs elevation", "BAD_PARAM", "'('"),
    ("2 $ elevation", "BAD_PARAM", "column 3"),
    (f"{A} ^ {B}", "UNSUPPORTED", ".^"),
    ("min(elevation)", "UNSUPPORTED", "min"),
    ("max(elevation)", "UNSUPPORTED", "not built"),
    ("transpose(elevation)", "UNSUPPORTED", "not built"),
    ("trace(elevation)", "UNSUPPORTED", "not built"),
    ("norm(elevation)", "UNSUPPORTED", "not built"),
    ("zeros(3, 3)", "UNSUPPORTED", "not built"),
    ("ones(3, 3)", "UNSUPPORTED", "not built"),
    ("eye(3)", "UNSUPPORTED", "not built"),
    ("elevation(1, 2)", "UNSUPPORTED", "indexing"),
    ("traversability = elevation", "UNSUPPORTED", "assignment"),
    ("elevation < 0.5", "UNSUPPORTED", "relational"),
    ("elevation == 0.5", "UNSUPPORTED", "relational"),
    ("elevation'", "UNSUPPORTED", "transpose"),
]


@pytest.mark.parametrize("text,kind,part", ERRORS, ids=[e[0][:40] or "empty" for e in ERRORS])
def test_every_refusal_arrives_with_its_class_and_a_column(exe, text, kind, part):
    got = status(exe, text)
    assert got[0] == "ERR" and got[1] == kind, got
    assert "column " in got[2] and part in got[2], got


def test_the_limits_themselves_are_accepted(exe):
    assert status(exe, "elevation" + " + elevation" * 31)[:2] == ["OK", "63"]
    s = status(exe, chain(7))
    assert s[0] == "OK" and s[2].split()[-1] == "8", s                                 # stack depth 8
    assert status(exe, " + ".join(R.LAYER_NAMES[:8]))[0] == "OK"
    assert status(exe, " + ".join(f"sum({n})" for n in R.LAYER_NAMES[:4]))[2].split()[1] == "4"
    assert status(exe, "(" * 60 + "elevation" + ")" * 60)[0] == "OK"
    assert status(exe, "(" * 70 + "elevation" + ")" * 70)[:2] == ["ERR", "BAD_PARAM"]


def test_constants_fold_through_arithmetic_only(exe):
    # (1.0 / 3.0) is one constant: push c, three pushes, two additions, one product
    assert status(exe, SHIPPED)[1] == "7"
    assert status(exe, "-(2 + 3 * 4 - 1 / 8) + elevation")[1] == "3"
    assert status(exe, "sqrt(4.0) + elevation")[1] == "4"    # never through a function
    assert status(exe, "2 ^ 2 + elevation")[1] == "5"        # nor through powf


def test_the_shipped_expression_reproduces_the_bag_layer(exe, tmp_path, bag):
    layers = {k: bag[k].reshape(1, -1) for k in (A, B, C)}
    got = run(exe, SHIPPED, layers, tmp_path)
    want = bag["traversability"].reshape(1, -1)
    assert got.shape == (1, 13300) and np.array_equal(np.isnan(got), np.isnan(want))
    assert R.same_bits(got, want)
    assert R.same_bits(R.evaluate(SHIPPED, layers), want)  # (and the numpy evaluator agrees with the reference's own result)
