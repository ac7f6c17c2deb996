"""Admission of the conditioning fixtures (tests/conditioning_cases.py), on the CPU: the oracle against the exact model of
the three filters (tests/ref_py/normals_ref.py).

The oracle restates NormalVectorsFilter's `sum(p p^T) / n - mean mean^T` on absolute coordinates bit for bit and so has
noise of its own at an altitude, on steep relief and far from the map origin.  A fixture may judge a kernel only if the
oracle ALONE stays within TOL / 4 of the exact model on every finite cell of slope, roughness and the combined layer and has
the model's NaN pattern: three quarters of the project's tolerance are then the kernel's.  A cell whose exact nz lies within
1e-3 float32 ulp of a rounding boundary AND on which the oracle rounded the other way is set apart -- there the last bit of
any solver decides, and one ulp of nz is worth up to 1e-5 of slope score --; a fixture may hold at most 3 such cells, the cap
tests/test_gpu_random.py applies.  (Being near a boundary alone sets nothing apart: two cells in a thousand are, about 50 on
a map of this size, and nearly all of them round the same way in both.)  A fixture
that fails is changed (lower altitude, more relief in the disc, coarser res), never the bound.  DESIGN.md section 7 records
the measured distances."""
import os
import subprocess

import numpy as np
import pytest

from tests import conditioning_cases as cc
from tests.conftest import ROOT
from tests.helpers import TOL
from tests.ref_py import normals_ref

ADMIT = TOL / 4
MAX_TIE_CELLS = 3
SCORES = ("traversability_slope", "traversability_roughness", "traversability")


def distance(oracle, name):
    """-> ({layer: max |oracle - model| off the cells set apart}, {layer: NaN-pattern mismatches}, cells set apart, cells
    near a rounding boundary)."""
    _, rows, cols, res, pos, elev, over = cc.case(name)
    over = dict(over)
    rank_rule = bool(over.pop("rank_rule", 0))
    op = oracle.default_params(**over)
    oracle.set_normals_rank_rule(rank_rule)
    try:
        want = oracle.chain(oracle.geom(rows, cols, res, pos), op, elev, want_normals=True)
    finally:
        oracle.set_normals_rank_rule(False)
    model = normals_ref.chain(rows, cols, res, pos, elev, op, want["traversability_step"], rank_rule)
    nan = {}
    near = np.zeros(rows * cols, bool)
    near[model["tie_cells"]] = True
    diff = {}
    for k in SCORES:
        a, b = want[k].reshape(-1), model[k].reshape(-1)
        nan[k] = int((np.isnan(a) != np.isnan(b)).sum())
        both = np.isfinite(a) & np.isfinite(b)
        diff[k] = np.where(both, np.abs(a.astype(np.float64) - b.astype(np.float64)), 0.0)
    # set apart: cells on a rounding boundary of nz where the oracle's last bit fell the other way
    # (slope, and the combined layer that holds a third of it: roughness has no rounding tie of nz to be forgiven)
    apart = near & (np.maximum(diff["traversability_slope"], diff["traversability"]) > ADMIT)
    dist = {k: float(diff[k][~apart].max()) for k in SCORES}
    return dist, nan, int(apart.sum()), int(near.sum())


@pytest.fixture(scope="module")
def threads(oracle):
    oracle.set_threads(min(os.cpu_count() or 1, 16))
    yield
    oracle.set_threads(1)


@pytest.mark.parametrize("name", cc.names())
def test_fixture_is_admitted(oracle, threads, name):
    dist, nan, ties, near = distance(oracle, name)
    print(f"{name}: " + ", ".join(f"{k} {dist[k]:.3g}" for k in SCORES) + f", tie cells {ties} (of {near} near a boundary)")
    assert all(v == 0 for v in nan.values()), (name, nan)
    assert ties <= MAX_TIE_CELLS, (name, ties)
    assert all(v <= ADMIT for v in dist.values()), (name, dist)


def test_model_on_a_known_plane():
    """z = a x + b y exactly (dyadic slopes and positions): the model's normal is (-a, -b, 1) / |.| to float32, the slope
    score follows, the roughness score is 1; an isolated cell and a pair give UnitZ."""
    rows, cols, res = 20, 24, 0.5
    j, i = np.mgrid[0:cols, 0:rows]
    a, b = 0.25, -0.5
    x = (0.5 * rows * res - 0.5 * res) - res * i
    y = (0.5 * cols * res - 0.5 * res) - res * j
    elev = (a * x + b * y + 100.0).astype(np.float32)
    elev[0:8, :] = np.nan
    elev[3, 4] = 100.0               # alone in its disc
    elev[3, 10] = elev[3, 11] = 7.0  # two points

    class P:
        normals_radius = rough_radius = 1.6
        normals_axis = 2
        slope_critical, rough_critical = 1.0, 0.05
        w_scale, w_slope, w_step, w_rough = 1.0 / 3.0, 1.0, 1.0, 1.0

    out = normals_ref.chain(rows, cols, res, (3.0, -2.0), elev.reshape(-1), P, np.ones(rows * cols, np.float32))
    n = np.array([-a, -b, 1.0]) / np.sqrt(a * a + b * b + 1.0)
    inner = np.zeros((cols, rows), bool)
    inner[12:-4, 4:-4] = True
    for k, name in enumerate(("surface_normal_x", "surface_normal_y", "surface_normal_z")):
        assert np.array_equal(out[name].reshape(cols, rows)[inner], np.full(inner.sum(), np.float32(n[k]))), name
    want_slope = np.float32(1.0 - np.arccos(np.float64(np.float32(n[2]))))
    assert np.all(out["traversability_slope"].reshape(cols, rows)[inner] == want_slope)
    assert np.abs(out["traversability_roughness"].reshape(cols, rows)[inner] - 1.0).max() < 1e-6
    for (jj, ii) in ((3, 4), (3, 10), (3, 11)):
        assert out["surface_normal_z"].reshape(cols, rows)[jj, ii] == 1.0
        assert out["traversability_slope"].reshape(cols, rows)[jj, ii] == 1.0
    assert out["traversability_roughness"].reshape(cols, rows)[3, 4] == 0.0   # one point: 0 / 0
    assert np.isnan(out["surface_normal_z"].reshape(cols, rows)[0, 0]) and np.isnan(out["traversability"].reshape(cols, rows)[0, 0])


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """The strip plan of a whole-map launch from the kernels' own header (tests/cpu/n3_plan_check.cpp, `plan` mode)."""
    exe = tmp_path_factory.mktemp("n3") / "n3_plan_check"
    src = os.path.join(ROOT, "tests", "cpu", "n3_plan_check.cpp")
    inc = os.path.join(ROOT, "traversability_estimation_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", inc, src, "-o", str(exe)], check=True, timeout=300)

    def ask(rows, cols, R, slots, maps, short=0):
        out = subprocess.run([str(exe), "plan"] + [str(int(v)) for v in (rows, cols, R, slots, maps, short)], capture_output=True,
                             text=True, check=True, timeout=60).stdout.split()
        return dict(zip(out[0::2], (int(v) for v in out[1::2])))
    return ask


SLOTS = [k * 256 for k in (9, 10, 11, 12)]  # resident single-wave blocks of a 256-CU device (te_normals3.hip: resident_blocks)


def _marching():
    for name, rows, cols, res, pos, elev, over in cc.cases():
        R = int(np.floor(over["normals_radius"] / res + 1e-9))
        if rows >= 64 and 3 <= R <= 10 and "rank_rule" not in over:
            yield name, rows, cols, R


def test_marching_fixtures_have_interior_block_columns(plan):
    """Only interior block columns run the closed-form tail, the TIES interior path and the hole queue: every fixture the
    marching kernels take must have one, alone and as one of a batch of two."""
    seen = 0
    for name, rows, cols, R in _marching():
        for slots in SLOTS:
            for maps in (1, 2):
                for short in (0, 1):
                    p = plan(rows, cols, R, slots, maps, short)
                    assert p["n_int"] >= 1 and p["s_int"] >= 1, (name, slots, maps, short, p)
        seen += 1
    assert seen >= 20


def test_long_strip_batches_get_long_strips(plan):
    """A batch of LONG_STRIP_MAPS copies of a 320-column fixture: interior strips of at least 80 rows whatever the slots."""
    for name in cc.LONG_STRIP:
        _, rows, cols, res, pos, elev, over = cc.case(name)
        R = int(np.floor(over["normals_radius"] / res + 1e-9))
        for slots in SLOTS:
            p = plan(rows, cols, R, slots, cc.LONG_STRIP_MAPS)
            assert p["n_int"] >= 1 and p["rows_int"] >= 80, (name, slots, p)
            assert plan(rows, cols, R, slots, 1)["rows_int"] <= 16, name  # (what one map alone gets)
