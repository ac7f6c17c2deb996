"""tests/ref_py/raster_normals_ref.py, the yardstick of the raster method of NormalVectorsFilter (include/travgpu.h,
TE_OPT_NORMALS_ALGORITHM): (a) its sign convention against the area method the bag pins, on exact planes; (b) vectors computed
by hand for every neighbour configuration of the contract."""
import itertools

import numpy as np
import pytest

from tests.ref_py import raster_normals_ref as R

NAN, INF = np.float32(np.nan), np.float32(np.inf)
RES = 0.5


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- (a) exact planes: the area method of the oracle gives the same normals -----------------------------------------------------

@pytest.mark.parametrize("a,b", [(0.25, -0.5), (-1.0, 0.0), (0.0, 2.0)])
def test_planes_give_the_area_methods_normals(oracle, a, b):
    """z = a x + b y on 12 x 9 at res 0.5 around a dyadic position: every elevation is exact in float32, the raster normal is
    (-a, -b, 1) normalised, and so is the PCA normal of the 3 x 3 disc (radius 1.5 res).  Interior cells, each component within
    one float32 ulp (the spacing at the expected value); the frame is NaN under raster and clipped discs under area."""
    rows, cols, pos = 12, 9, (0.75, -1.25)
    g = oracle.geom(rows, cols, RES, pos)
    x = pos[0] + (0.5 * rows * RES - 0.5 * RES) - RES * np.arange(rows)  # x grows towards smaller i
    y = pos[1] + (0.5 * cols * RES - 0.5 * RES) - RES * np.arange(cols)
    z = (a * x[:, None] + b * y[None, :]).astype(np.float32)
    assert np.array_equal(z.astype(np.float64), a * x[:, None] + b * y[None, :])
    want = [R.as_matrix(v, rows, cols) for v in oracle.normals(g, R.as_flat(z), 1.5 * RES, 2)]
    got = R.raster_normals(z, RES, 2)
    norm = np.sqrt(a * a + b * b + 1.0)
    for k, expect in enumerate(((0.0 - a) / norm, (0.0 - b) / norm, 1.0 / norm)):  # (a difference: no negative zero)
        gi, wi = got[k][1:-1, 1:-1], want[k][1:-1, 1:-1]
        assert np.isfinite(gi).all() and np.isfinite(wi).all()
        ulp = np.spacing(np.abs(wi))
        print(f"plane ({a}, {b}) component {k}: max |raster - area| = {np.abs(gi.astype(np.float64) - wi).max():.3g}, ulp {ulp.max():.3g}")
        assert (np.abs(gi.astype(np.float64) - wi.astype(np.float64)) <= ulp).all(), k
        assert (gi == np.float32(expect)).all(), k  # (as values: a row at x = 0 holds zeros of both signs)
    for v in got:  # rule 1
        frame = np.ones((rows, cols), bool)
        frame[1:-1, 1:-1] = False
        assert np.isnan(v[frame]).all()


# ---- (b) hand-computed vectors ----------------------------------------------------------------------------------------------------
# res = 0.5, centre c = 5.  x direction, wanted gradient +2:  both: t = 0, b = 2 -> (2 - 0) / (2 * 0.5); only t: t = 4 -> (5 - 4) / 0.5;
# only b: b = 6 -> (6 - 5) / 0.5.  y direction, wanted gradient -2: both: l = 2, r = 0; only l: l = 6 -> (5 - 6) / 0.5; only r: r = 4.
# n = (2, -2, 1) / sqrt((4 + 4) + 1) = (2/3, -2/3, 1/3).
X_CONFIGS = {"both": (0.0, 2.0), "only_t": (4.0, NAN), "only_b": (NAN, 6.0)}
Y_CONFIGS = {"both": (2.0, 0.0), "only_l": (6.0, NAN), "only_r": (NAN, 4.0)}
THIRDS = (np.float32(2.0 / 3.0), np.float32(-2.0 / 3.0), np.float32(1.0 / 3.0))


def cross(c, t, b, l, r):
    """3 x 3 map with the given centre and four neighbours; the corners hold a value no rule may read."""
    z = np.full((3, 3), 1e30, np.float32)
    z[1, 1], z[0, 1], z[2, 1], z[1, 0], z[1, 2] = c, t, b, l, r
    return z


def centre(z, axis=2):
    out = R.raster_normals(z, RES, axis)
    for v in out:  # 3 x 3: the centre is the only cell visited
        frame = np.ones((3, 3), bool)
        frame[1, 1] = False
        assert np.isnan(v[frame]).all()
    return tuple(v[1, 1] for v in out)


@pytest.mark.parametrize("xc,yc", list(itertools.product(X_CONFIGS, Y_CONFIGS)))
def test_the_nine_neighbour_configurations(xc, yc):
    (t, b), (l, r) = X_CONFIGS[xc], Y_CONFIGS[yc]
    got = centre(cross(5.0, t, b, l, r))
    assert np.array_equal(bits(got), bits(THIRDS)), (xc, yc, got)


def test_one_sided_differences_need_the_centre():
    for (xc, yc) in itertools.product(X_CONFIGS, Y_CONFIGS):
        (t, b), (l, r) = X_CONFIGS[xc], Y_CONFIGS[yc]
        got = centre(cross(NAN, t, b, l, r))
        if (xc, yc) == ("both", "both"):  # an invalid centre between two finite pairs does get a normal
            assert np.array_equal(bits(got), bits(THIRDS))
        else:
            assert np.isnan(got).all(), (xc, yc)


def test_a_direction_without_a_neighbour_gives_nan():
    assert np.isnan(centre(cross(5.0, NAN, NAN, 2.0, 0.0))).all()
    assert np.isnan(centre(cross(5.0, 0.0, 2.0, NAN, NAN))).all()
    assert np.isnan(centre(cross(NAN, NAN, NAN, NAN, NAN))).all()


@pytest.mark.parametrize("inf", [INF, -INF])
def test_infinite_cells_count_as_missing(inf):
    # t = +-inf: only b is finite -> (6 - 5) / 0.5 = 2;  r = +-inf: only l -> (5 - 6) / 0.5 = -2
    assert np.array_equal(bits(centre(cross(5.0, inf, 6.0, 6.0, inf))), bits(THIRDS))
    # an infinite centre between finite pairs: the central differences do not read it
    assert np.array_equal(bits(centre(cross(inf, 0.0, 2.0, 2.0, 0.0))), bits(THIRDS))
    # ... and one-sided differences cannot use it
    assert np.isnan(centre(cross(inf, 4.0, NAN, 2.0, 0.0))).all()


def test_the_three_positive_axes():
    z = cross(5.0, 0.0, 2.0, 2.0, 0.0)  # n = (2/3, -2/3, 1/3)
    assert np.array_equal(bits(centre(z, 2)), bits(THIRDS))
    assert np.array_equal(bits(centre(z, 0)), bits(THIRDS))  # the x component is positive already
    assert np.array_equal(bits(centre(z, 1)), bits(tuple(-v for v in THIRDS)))  # the y component is negative: n = -n
    zx = cross(5.0, 2.0, 0.0, 2.0, 0.0)  # gx = -2: n = (-2/3, -2/3, 1/3)
    assert np.array_equal(bits(centre(zx, 0)), bits((THIRDS[0], THIRDS[0], THIRDS[1] / 2)))
    assert np.array_equal(bits(centre(zx, 2)), bits((THIRDS[1], THIRDS[1], THIRDS[2])))
    # a level cell: (0, 0, 1); on the x axis 0 is not < 0: no flip, no negative zero
    flat = cross(5.0, 5.0, 5.0, 5.0, 5.0)
    for axis in (0, 1, 2):
        assert np.array_equal(bits(centre(flat, axis)), bits((0.0, 0.0, 1.0)))
    # a 3-4-5 slope: gx = 0.75 -> (0.75, 0, 1) / 1.25 = (0.6, 0, 0.8)
    assert np.array_equal(bits(centre(cross(0.0, 0.0, 0.75, 1.0, 1.0))), bits((np.float32(0.6), 0.0, np.float32(0.8))))


@pytest.mark.parametrize("rows,cols", [(2, 7), (7, 2), (1, 1), (1, 5)])
def test_maps_without_an_interior_are_all_nan(rows, cols):
    z = np.arange(rows * cols, dtype=np.float32).reshape(rows, cols)
    for v in R.raster_normals(z, RES):
        assert v.shape == (rows, cols) and v.dtype == np.float32 and np.isnan(v).all()


def test_flat_layers_are_column_major():
    rows, cols = 5, 4
    z = np.random.default_rng(3).normal(size=(rows, cols)).astype(np.float32)
    flat = R.as_flat(z)
    assert flat[2 * rows + 3] == z[3, 2] and np.array_equal(R.as_matrix(flat, rows, cols), z)
    for a, b in zip(R.raster_normals_flat(flat, rows, cols, RES), R.raster_normals(z, RES)):
        assert np.array_equal(bits(a), bits(R.as_flat(b)))
