"""Exact model of NormalVectorsFilter (area, serial), SlopeFilter and RoughnessFilter for small maps.

TEST INFRASTRUCTURE (numpy, maps of a few ten thousand cells).  Written from the filters' published algorithm
(grid_map_filters NormalVectorsFilter::areaSingleNormalComputation, traversability_estimation_filters
SlopeFilter.cpp:59-88, RoughnessFilter.cpp:73-132) and independent of oracle/te_oracle.c and of the kernels' headers.
Where the filter forms `sum(p p^T) / n - mean mean^T` on ABSOLUTE coordinates -- and so loses digits to the altitude and
to the map position --, this model takes every point relative to the disc's centre cell and forms the two-pass centred
covariance `sum((p - mean)(p - mean)^T) / n` in np.longdouble: neither altitude nor map origin enters its arithmetic.
What it yields is what the filter would yield in exact arithmetic, to the last float32 bit except where a value lies
on a rounding boundary (`tie_cells`); the distance of the oracle from it is the reference's own noise.

Disc membership is grid_map's CircleIterator as tests/ref_py/grid_map_ref.py restates it (rounded cell positions, so
the cells on the circle of a whole-cell radius belong to a disc or not centre by centre); it is evaluated here with
shifted views over the whole map and checked against GridMapRef.circle itself on the map's border and on a scatter of
interior centres every time a model is built.

Layers are flat float32 arrays in grid_map storage order, value(i, j) = a[j * rows + i].
"""
import numpy as np

from tests.ref_py.grid_map_ref import GridMapRef

LD = np.longdouble


def _positions(gm):
    """Cell-centre coordinates along i and j, the very float operations of GridMapRef.position."""
    out = []
    for k in (0, 1):
        idx = np.arange(gm.size[k], dtype=np.float64)
        out.append(gm.pos[k] + (0.5 * gm.length[k] - 0.5 * gm.res) + gm.res * (-idx))
    return out


class Discs:
    """Membership of every offset (di, dj) in the disc of every centre: `masks()` yields (di, dj, inside[cols, rows])
    where inside[j, i] says that cell (i + di, j + dj) is in the map and in the disc of centre (i, j)."""

    def __init__(self, rows, cols, res, pos, radius, check=True):
        self.gm = GridMapRef(rows, cols, res, pos)
        self.rows, self.cols, self.radius = rows, cols, float(radius)
        self.px, self.py = _positions(self.gm)
        self.K = int(np.floor(radius / res + 1e-9)) + 1  # one ring beyond: its cells must all come out False
        if check:
            self._check_against_the_iterator()

    def inside(self, di, dj):
        rows, cols = self.rows, self.cols
        r2 = self.radius * self.radius
        out = np.zeros((cols, rows), bool)
        i0, i1 = max(0, -di), min(rows, rows - di)
        j0, j1 = max(0, -dj), min(cols, cols - dj)
        if i0 >= i1 or j0 >= j1:
            return out
        dx = self.px[i0 + di:i1 + di] - self.px[i0:i1]
        dy = self.py[j0 + dj:j1 + dj] - self.py[j0:j1]
        out[j0:j1, i0:i1] = dx[None, :] * dx[None, :] + dy[:, None] * dy[:, None] <= r2
        return out

    def masks(self):
        for dj in range(-self.K, self.K + 1):
            for di in range(-self.K, self.K + 1):
                m = self.inside(di, dj)
                if m.any():
                    yield di, dj, m

    def _check_against_the_iterator(self):
        rows, cols = self.rows, self.cols
        rng = np.random.default_rng(rows * 1009 + cols)
        centres = {(0, 0), (rows - 1, 0), (0, cols - 1), (rows - 1, cols - 1), (rows // 2, cols // 2)}
        centres |= {(int(rng.integers(0, rows)), int(rng.integers(0, cols))) for _ in range(24)}
        centres |= {(int(rng.integers(0, rows)), int(rng.choice([0, 1, cols - 2, cols - 1]))) for _ in range(8)}
        centres |= {(int(rng.choice([0, 1, rows - 2, rows - 1])), int(rng.integers(0, cols))) for _ in range(8)}
        centres = {(min(max(i, 0), rows - 1), min(max(j, 0), cols - 1)) for i, j in centres}
        mine = {c: set() for c in centres}
        for di, dj, m in self.masks():
            for (i, j) in centres:
                if m[j, i]:
                    mine[(i, j)].add((i + di, j + dj))
        for c in centres:
            theirs = set(self.gm.circle(self.gm.position(c), self.radius))
            assert mine[c] == theirs, ("disc membership differs from CircleIterator", c, sorted(mine[c] ^ theirs))


def _shift(a, di, dj):
    """b[j, i] = a[j + dj, i + di] where that cell exists, 0 elsewhere (the membership mask never selects those)."""
    cols, rows = a.shape
    b = np.zeros_like(a)
    i0, i1 = max(0, -di), min(rows, rows - di)
    j0, j1 = max(0, -dj), min(cols, cols - dj)
    if i0 < i1 and j0 < j1:
        b[j0:j1, i0:i1] = a[j0 + dj:j1 + dj, i0 + di:i1 + di]
    return b


def _points(discs, z, valid, res):
    """(use, x, y, dz) per disc offset: which centres hold a valid point there, and its coordinates relative to the
    centre cell -- x = -res * di, y = -res * dj, dz = z - z(centre) -- as longdouble."""
    r = LD(res)
    for di, dj, m in discs.masks():
        use = m & _shift(valid, di, dj)
        if use.any():
            yield use, -r * LD(di), -r * LD(dj), np.where(use, _shift(z, di, dj) - z, LD(0))


def _moments(discs, z, valid, res):
    """Two passes over the disc offsets: count, mean and centred second moments (longdouble) of every disc's valid points."""
    shape = z.shape
    n = np.zeros(shape, np.int64)
    s = [np.zeros(shape, LD) for _ in range(3)]
    for use, x, y, dz in _points(discs, z, valid, res):
        n += use
        s[0] += np.where(use, x, LD(0))
        s[1] += np.where(use, y, LD(0))
        s[2] += dz
    nn = np.maximum(n, 1).astype(LD)
    mean = [v / nn for v in s]
    c = {k: np.zeros(shape, LD) for k in ("xx", "xy", "xz", "yy", "yz", "zz")}
    for use, x, y, dz in _points(discs, z, valid, res):
        qx = np.where(use, x - mean[0], LD(0))
        qy = np.where(use, y - mean[1], LD(0))
        qz = np.where(use, dz - mean[2], LD(0))
        c["xx"] += qx * qx
        c["xy"] += qx * qy
        c["xz"] += qx * qz
        c["yy"] += qy * qy
        c["yz"] += qy * qz
        c["zz"] += qz * qz
    return n, mean, c


def normals(rows, cols, res, pos, elev, radius, axis=2, rank_rule=False):
    """-> dict: surface_normal_x/_y/_z (flat float32, NaN where the centre is invalid), nz64 (the z component before it is
    rounded) and tie_cells (flat indices of cells whose nz64 lies within 1e-3 float32 ulp of a rounding boundary)."""
    z32 = np.asarray(elev, np.float32).reshape(cols, rows)
    valid = np.isfinite(z32)
    z = np.where(valid, z32, 0).astype(LD)
    discs = Discs(rows, cols, res, pos, radius)
    n, _, c = _moments(discs, z, valid, res)  # (an invalid centre yields no output: its dz are never used)
    nn = np.maximum(n, 1).astype(LD)
    cov = np.empty(z.shape + (3, 3), np.float64)
    for (a, b), k in {(0, 0): "xx", (0, 1): "xy", (0, 2): "xz", (1, 1): "yy", (1, 2): "yz", (2, 2): "zz"}.items():
        cov[..., a, b] = cov[..., b, a] = (c[k] / nn).astype(np.float64)
    w, v = np.linalg.eigh(cov)  # ascending; the centred matrix is well conditioned
    nv = v[..., :, 0].copy()
    unit_z = (n < 3) | ~(w[..., 1] > 1e-8)
    if rank_rule:
        # rank of the centred scatter matrix below 3.  Only inputs with a wide margin are meant (an exact plane, or a plane
        # with noise far above rounding): between them lies a band that neither the filter nor this model defines.
        unit_z |= ~(w[..., 0] > 1e-10 * w[..., 2])
    nv[unit_z] = (0.0, 0.0, 1.0)
    flip = nv[..., axis] < 0.0
    nv[flip] = -nv[flip]
    out = {}
    for k, name in enumerate(("surface_normal_x", "surface_normal_y", "surface_normal_z")):
        out[name] = np.where(valid, nv[..., k], np.nan).astype(np.float32).reshape(-1)
    nz64 = np.where(valid, nv[..., 2], np.nan)
    out["nz64"] = nz64.reshape(-1)
    out["tie_cells"] = np.flatnonzero(_ulps_from_a_rounding_boundary(nz64.reshape(-1)) < 1e-3)
    return out


def _ulps_from_a_rounding_boundary(x):
    """Distance of each double from the nearest midpoint of two neighbouring float32 values, in float32 ulps."""
    x = np.asarray(x, np.float64)
    f = x.astype(np.float32)
    up = np.nextafter(f, np.float32(np.inf)).astype(np.float64)
    dn = np.nextafter(f, np.float32(-np.inf)).astype(np.float64)
    f = f.astype(np.float64)
    ulp = np.maximum(up - f, f - dn)
    d = np.minimum(np.abs(x - 0.5 * (f + up)), np.abs(x - 0.5 * (f + dn))) / ulp
    return np.where(np.isfinite(x), d, np.inf)


def slope(nz32, critical):
    """SlopeFilter.cpp:59-88 on the stored (float32) nz."""
    nz = np.asarray(nz32, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        s = np.arccos(nz)
        score = np.where(s < critical, 1.0 - s / critical, 0.0)
    return np.where(np.isfinite(nz), score, np.nan).astype(np.float32)


def roughness(rows, cols, res, pos, elev, nrm, radius, critical):
    """RoughnessFilter.cpp:73-132 with the stored (float32) normal: sqrt(sum(dist^2) / (n - 1)) of the disc's valid points
    from the plane through their mean; a disc of one point gives 0 / 0 and so the score 0."""
    z32 = np.asarray(elev, np.float32).reshape(cols, rows)
    valid = np.isfinite(z32)
    z = np.where(valid, z32, 0).astype(LD)
    a = [np.asarray(nrm[k], np.float32).reshape(cols, rows) for k in ("surface_normal_x", "surface_normal_y", "surface_normal_z")]
    have = np.isfinite(a[0])
    ax, ay, az = (np.where(have, v, 0).astype(LD) for v in a)
    discs = Discs(rows, cols, res, pos, radius)
    n, mean, _ = _moments(discs, z, valid, res)
    total = np.zeros(z.shape, LD)
    for use, x, y, dz in _points(discs, z, valid, res):
        d = np.where(use, ax * (x - mean[0]) + ay * (y - mean[1]) + az * (dz - mean[2]), LD(0))
        total += d * d
    with np.errstate(invalid="ignore", divide="ignore"):
        rough = np.sqrt(total / (n - 1).astype(LD)).astype(np.float64)  # n = 1: 0 / 0
        score = np.where(rough < critical, 1.0 - rough / critical, 0.0)
    return np.where(have, score, np.nan).astype(np.float32).reshape(-1)


def combine(p, slope_l, step_l, rough_l):
    """The chain's MathExpressionFilter in float32, left to right: w_scale * (w_slope * slope + w_step * step + w_rough * rough)."""
    f = np.float32
    a = f(p.w_slope) * np.asarray(slope_l, f)
    b = f(p.w_step) * np.asarray(step_l, f)
    c = f(p.w_rough) * np.asarray(rough_l, f)
    return (f(p.w_scale) * ((a + b) + c)).astype(f)


def chain(rows, cols, res, pos, elev, p, step_layer, rank_rule=False):
    """Normals, slope, roughness and the combined layer of parameters `p` (an oracle Params or anything with its field
    names); the step layer -- float comparisons, nothing to model -- is given."""
    nrm = normals(rows, cols, res, pos, elev, p.normals_radius, p.normals_axis, rank_rule)
    out = dict(nrm)
    out["traversability_slope"] = slope(nrm["surface_normal_z"], p.slope_critical).reshape(-1)
    out["traversability_roughness"] = roughness(rows, cols, res, pos, elev, nrm, p.rough_radius, p.rough_critical)
    out["traversability_step"] = np.asarray(step_layer, np.float32).reshape(-1)
    out["traversability"] = combine(p, out["traversability_slope"], out["traversability_step"], out["traversability_roughness"])
    return out
