"""The yardsticks of tests/test_gpu_plugin_filters.py against each other, without a GPU: the oracle's single filters
(oracle.normals / slope / roughness / combine, thin wrappers over oracle/te_oracle.c) fed the oracle's own layers are
oracle.chain bit for bit, and fed foreign normals they are the numpy restatement of tests/ref_py/plugin_filters_ref.py on every
cell: the same NaN cells, the same zeros, values within one float32 ulp (both are float64 computations in another order of
summation, each rounded once to float32).  The critical values keep every cell clear of the threshold, which the tests assert
of their own inputs, so no cell is left out."""
import numpy as np
import pytest

from tests import plugin_filter_cases as K
from tests.ref_py import plugin_filters_ref as R

SHAPES = [(40, 31), (9, 50)]
RADII = [2.5, 2, 5.4]  # cells: tie-free, a whole-cell radius, wider than the 9-row map
FOREIGN = [k for k in K.NORMAL_KINDS if k != "own"]
CLEAR = 1e-12


def _bits(a):
    return np.asarray(a, np.float32).reshape(-1).view(np.uint32)


def _elev(rows, cols, seed, kind=None, cells=0.0):
    t = K.terrain(rows, cols, seed)
    return (K.void(t, np.ceil(cells)) if kind == "void" else K.punch(t, seed + 1)).reshape(-1)


def _one_ulp(a, b):
    """|a - b| <= one float32 ulp of the larger magnitude, on the cells where both are finite."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ok = np.isfinite(a) & np.isfinite(b)
    big = np.maximum(np.abs(a[ok]), np.abs(b[ok]))
    return np.abs(a[ok].astype(np.float64) - b[ok].astype(np.float64)) <= np.spacing(big).astype(np.float64)


@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("cells", RADII)
def test_single_filters_on_own_layers_are_the_chain(oracle, rows, cols, cells):
    elev = _elev(rows, cols, 300 + rows)
    g = oracle.geom(rows, cols, K.RES, (0.3, -0.2))
    op = oracle.default_params(normals_radius=cells * K.RES, rough_radius=cells * K.RES, step_radius1=2.5 * K.RES, step_radius2=2 * K.RES)
    want = oracle.chain(g, op, elev, want_normals=True)
    nx, ny, nz = oracle.normals(g, elev, op.normals_radius, op.normals_axis)
    for k, a in (("surface_normal_x", nx), ("surface_normal_y", ny), ("surface_normal_z", nz)):
        assert np.array_equal(_bits(a), _bits(want[k])), k
    slope = oracle.slope(g, nz, op.slope_critical)
    rough = oracle.roughness(g, elev, nx, ny, nz, op.rough_critical, op.rough_radius)
    step = oracle.step(g, elev, op.step_critical, op.step_radius1, op.step_radius2, op.step_ncrit)
    assert np.array_equal(_bits(slope), _bits(want["traversability_slope"]))
    assert np.array_equal(_bits(rough), _bits(want["traversability_roughness"]))
    assert np.array_equal(_bits(step), _bits(want["traversability_step"]))
    trav = oracle.combine(slope, step, rough, op.w_scale, op.w_slope, op.w_step, op.w_rough)
    assert np.array_equal(_bits(trav), _bits(want["traversability"]))
    assert np.isfinite(want["traversability"]).sum() > rows * cols // 2


@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("cells", RADII)
@pytest.mark.parametrize("kind", FOREIGN)
def test_roughness_of_foreign_normals(oracle, rows, cols, cells, kind):
    pos = (0.3, -0.2)
    elev = _elev(rows, cols, 500 + rows, kind, cells)
    nx, ny, nz = K.normals(kind, elev, None, 600 + cols)
    radius = cells * K.RES
    value, count = R.roughness_value(elev, nx, ny, nz, rows, cols, K.RES, radius, pos)
    # (a critical value that leaves about 70 % of the finite cells a non-zero score -- tilted normals are rougher than 0.05)
    some = value[np.isfinite(value) & (value > 0)]
    crit = float(np.quantile(some, 0.7)) * 1.0000123 if some.size >= 10 else 0.0437
    assert not (np.abs(value - crit) < CLEAR).any(), "a cell of the input sits on the critical value"
    want = R.roughness_given(elev, nx, ny, nz, rows, cols, K.RES, radius, crit, pos)
    got = oracle.roughness(oracle.geom(rows, cols, K.RES, pos), elev, nx, ny, nz, crit, radius)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.isnan(got), ~np.isfinite(nx))  # the reference tests surface_normal_x alone
    assert np.array_equal(got == 0, want == 0)
    assert _one_ulp(got, want).all()
    # the kind is what it says
    seen = np.isfinite(nx)
    if kind == "void":
        assert (count[seen] == 0).any() and (got[seen & (count == 0)] == 1.0).all()  # no point: 0 / (unsigned)(0 - 1)
        assert (count[seen] == 1).any() and (got[seen & (count == 1)] == 0.0).all()  # one point: 0 / 0
    else:
        assert (seen & ~np.isfinite(elev)).any()  # valid normals over invalid centres
        assert ((got > 0) & (got < 1)).sum() > rows * cols // 4
    if kind == "nan_nx":
        assert 0 < (~seen).sum() < seen.sum()
    if kind == "nan_ny":
        assert np.isnan(ny).any() and (got[np.isnan(ny)] == 0.0).all()
    if kind == "horizontal":
        assert (nz == 0).all()


def test_slope_of_foreign_normals(oracle):
    crit = float(oracle.default_params().slope_critical)
    for name, (rows, cols, maps) in K.slope_layers(crit).items():
        for nz in maps:
            angle = R.slope_angle(nz)
            assert not (np.abs(angle - crit) < CLEAR).any(), "a cell of the input sits on the critical angle"
            want = R.slope_from_nz(nz, crit)
            got = oracle.slope(oracle.geom(rows, cols, K.RES), nz, crit)
            assert np.array_equal(np.isnan(got), np.isnan(want)), name
            assert np.array_equal(np.isnan(got), ~np.isfinite(nz)), name
            assert np.array_equal(got == 0, want == 0), name
            assert _one_ulp(got, want).all(), name
            assert (got[nz == 1.0] == 1.0).all() and (got[np.abs(nz) > 1.0][np.isfinite(nz[np.abs(nz) > 1.0])] == 0.0).all()
            assert (got[nz == -1.0] == 0.0).all()
    # the table's three cells at the threshold fall on both sides of it
    t = K.slope_values(crit)
    s = oracle.slope(oracle.geom(t.size, 1, K.RES), t, crit)
    assert (s[9:12] == 0).any() and (s[9:12] > 0).any()
