"""The yardsticks and the inputs of tests/test_gpu_param_routes.py, without a GPU: oracle.combine is the float32 statement of
tests/ref_py/normals_ref.py bit for bit under every weight set, oracle.normals follows normal_vector_positive_axis as the numpy
model does, and every case of tests/param_route_cases.py is what it says -- the axis matters on an axis case's map and almost no
cell's sign is left to rounding, the footprint differs between the gap values (beyond the default growth on the region case), and
exchanging two weights changes the combined layer of every weight case."""
import itertools
import types

import numpy as np
import pytest

from tests import param_route_cases as P
from tests.ref_py import normals_ref

NRM = ("surface_normal_x", "surface_normal_y", "surface_normal_z")
AXIS_MAPS = [c for c in P.AXIS if c.axis == 0]  # (both axes of a template see the same map)


def _bits(a):
    return np.asarray(a, np.float32).reshape(-1).view(np.uint32)


def _ids(cases):
    return [P.case_id(c) for c in cases]


def _chain(oracle, c, elev, **over):
    oracle.set_normals_rank_rule(c.kind == "rank")
    try:
        return oracle.chain(oracle.geom(c.rows, c.cols, c.res, P.POS), P.params(oracle, c, **over), elev, want_normals=True)
    finally:
        oracle.set_normals_rank_rule(False)


@pytest.mark.parametrize("name", sorted(P.WEIGHT_SETS))
def test_combine_is_the_float32_statement(oracle, name):
    w = P.WEIGHT_SETS[name]
    rng = np.random.default_rng(11)
    layers = [rng.uniform(0.0, 1.0, 5000).astype(np.float32) for _ in range(3)]
    for k, a in enumerate(layers):
        a[rng.random(a.size) < 0.05] = np.nan
        a[rng.random(a.size) < 0.1] = k % 2  # the clips
    p = types.SimpleNamespace(w_scale=np.float32(w[0]), w_slope=np.float32(w[1]), w_step=np.float32(w[2]), w_rough=np.float32(w[3]))
    want = normals_ref.combine(p, *layers)
    got = oracle.combine(*layers, *w)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.isnan(got), np.isnan(layers[0]) | np.isnan(layers[1]) | np.isnan(layers[2]))  # 0 * NaN is NaN
    ok = ~np.isnan(got)
    assert np.array_equal(_bits(got[ok]), _bits(want[ok]))
    if name != "signed":  # (the signed set runs on k_combine alone, without the footprint)
        assert (abs(w[0]) * (abs(w[1]) + abs(w[2]) + abs(w[3])) <= 1.0) and len(set(w)) == 4
        assert 0.0 <= P.weights_cap(w) <= P.weights_cap(P.DEFAULT_WEIGHTS) + 1e-7  # the footprint's route: as under the defaults


def _final_maps(c):
    """The maps a case ends on: a region case's map before and after its tile, the observed maps of a batch."""
    maps = P.elevation(c)
    if c.kind == "region":
        r0, c0, h, w = c.region
        after = maps[0].copy()
        after[c0:c0 + w, r0:r0 + h] = P.tile(c, maps[0])
        maps = [maps[0], after]
    return [e for e in maps if np.isfinite(e).any()]


# (the rank-rule map is left out: the model's rank rule is defined only far from the band between an exact plane and a noisy
# one -- tests/ref_py/normals_ref.py --, and the map's plateau edges lie in it)
MODEL_MAPS = [c for c in AXIS_MAPS if c.kind != "rank"]


@pytest.mark.parametrize("c", MODEL_MAPS, ids=lambda c: P.case_id(c))
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_oracle_normals_follow_the_axis_as_the_model_does(oracle, c, axis):
    """oracle.normals(axis) against the numpy model on every axis case's maps: differences within 1e-5 (the tolerance of the
    restatement tests), the cells whose sign rounding decides left to either sign."""
    from tests.helpers import orient_axis_normals
    g = oracle.geom(c.rows, c.cols, c.res, P.POS)
    radius = c.cells[0] * c.res
    for e in _final_maps(c):
        got = dict(zip(NRM, oracle.normals(g, e, radius, axis)))
        want = normals_ref.normals(c.rows, c.cols, c.res, P.POS, e, radius, axis)
        free = P.sign_free(c._replace(axis=axis), e, got)
        a, b = orient_axis_normals(got, got, free), orient_axis_normals(want, got, free)
        for k in NRM:
            assert np.array_equal(np.isnan(a[k]), np.isnan(b[k])), k
            ok = ~np.isnan(a[k])
            assert np.abs(a[k][ok].astype(np.float64) - b[k][ok]).max() <= 1e-5, (k, axis)
        assert (got[NRM[axis]][~np.isnan(got[NRM[axis]])] >= 0).all()


@pytest.mark.parametrize("c", P.AXIS, ids=_ids(P.AXIS))
def test_the_axis_matters_on_every_axis_case(oracle, c):
    """Between 20 % and 80 % of the valid cells have surface_normal_z < 0 under the case's axis, and at most 0.2 % of them are
    sign-free (tests/param_route_cases.py: sign_free)."""
    for e in _final_maps(c):
        valid = np.isfinite(e).reshape(-1)
        want = _chain(oracle, c, e)
        down = (want["surface_normal_z"] < 0).sum() / valid.sum()
        free = P.sign_free(c, e, want).sum() / valid.sum()
        print(P.case_id(c), "nz < 0 on %.1f %%, sign-free %.3f %%" % (100 * down, 100 * free))
        assert 0.2 <= down <= 0.8, down
        assert free <= 0.002, free


def _footprint(oracle, c, elev, gap):
    g = oracle.geom(c.rows, c.cols, c.res, P.POS)
    op = P.params(oracle, c, fp_max_gap=gap)
    return oracle.footprint(g, op, elev, oracle.chain(g, op, elev))


def _differ(a, b):
    return (np.isnan(a) != np.isnan(b)) | (~np.isnan(a) & ~np.isnan(b) & (a != b))


def test_the_gap_values_give_different_footprints(oracle):
    c = P.GAP[0]
    elev = P.elevation(c)[0]
    fps = [_footprint(oracle, c, elev, gap) for gap in P.GAPS]
    for (ga, a), (gb, b) in zip(zip(P.GAPS, fps), list(zip(P.GAPS, fps))[1:]):
        n = int(_differ(a, b).sum())
        print("fp_max_gap %g against %g: %d cells differ" % (ga, gb, n))
        assert n >= 5, (ga, gb, n)
    for cc in P.GAP:  # (every gap case is that map)
        assert np.array_equal(_bits(np.nan_to_num(P.elevation(cc)[0])), _bits(np.nan_to_num(elev)))


def test_the_region_gap_case_changes_cells_beyond_the_default_growth(oracle):
    c = P.GAP_REGION
    elev = P.elevation(c)[0]
    r0, c0, h, w = c.region
    after = elev.copy()
    after[c0:c0 + w, r0:r0 + h] = P.tile(c, elev)
    changed = _differ(_footprint(oracle, c, elev, c.gap), _footprint(oracle, c, after, c.gap)).reshape(c.cols, c.rows)
    k = P.DEFAULT_GAP_GROWTH
    assert k == int(np.ceil(0.3 / c.res)) + 5
    outside = changed.copy()
    outside[max(0, c0 - k):c0 + w + k, max(0, r0 - k):r0 + h + k] = False
    print("footprint cells changed: %d, of them %d beyond %d cells of the tile" % (changed.sum(), outside.sum(), k))
    assert outside.sum() >= 5


@pytest.mark.parametrize("c", P.WEIGHTS, ids=_ids(P.WEIGHTS))
def test_exchanging_two_weights_changes_every_weight_case(oracle, c):
    maps = P.elevation(c)
    if c.kind == "region":
        r0, c0, h, w = c.region
        maps[0][c0:c0 + w, r0:r0 + h] = P.tile(c, maps[0])
    s = {k: [] for k in ("traversability_slope", "traversability_step", "traversability_roughness", "traversability")}
    for e in maps:
        for k, v in _chain(oracle, c, e).items():
            if k in s:
                s[k].append(v)
    s = {k: np.concatenate(v) for k, v in s.items()}
    if c.lone:  # the pairs' discs hold two points: the cells the route of any radius leaves to its exact kernel
        n = P.disc_points(c, maps[0], c.cells[0] * c.res)
        for j, i in P.LONE_PAIRS:
            assert n[j, i] == 2 and n[j, i + 1] == 2 and np.isfinite(s["traversability"].reshape(c.cols, c.rows)[j, i:i + 2]).all()
    w = c.weights
    finite = ~np.isnan(s["traversability"])
    assert finite.sum() >= 20
    for a, b in itertools.combinations((1, 2, 3), 2):
        x = list(w)
        x[a], x[b] = x[b], x[a]
        other = oracle.combine(s["traversability_slope"], s["traversability_step"], s["traversability_roughness"], *x)
        share = (other[finite] != s["traversability"][finite]).sum() / finite.sum()
        assert share >= 0.1, (a, b, share)
