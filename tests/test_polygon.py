"""Polygon footprints: TraversabilityMap::isTraversable(polygon) (TraversabilityMap.cpp:586-645) and
traversabilityFootprint(footprintYaw) (:239-305).  The C oracle against an independent pure-Python restatement on
small maps (CPU); the HIP kernels against the oracle, bit for bit (GPU, through the C-ABI)."""
import math

import numpy as np
import pytest

from tests.helpers import OUT_LAYERS, to_te_params
from tests.polygon_cases import EXISTING, FOOTPRINT, POINTS_XYZ, terrain  # noqa: F401  (other test modules import them from here)


def chain_layers(oracle, g, p, elev):
    return oracle.chain(g, p, elev)


# ---------------------------------------------------------------- pure-Python restatement
def py_bound(position, length, mappos):
    shifted = position - mappos + 0.5 * length
    eps = 10.0 * 2.220446049250313e-16
    if abs(position) > 1.0:
        eps *= abs(position)
    if shifted <= 0:
        shifted = eps
    elif shifted >= length:
        shifted = length - eps
    return shifted + mappos - 0.5 * length


def py_inside(verts, px, py):
    cross = 0
    n = len(verts)
    j = n - 1
    for i in range(n):
        xi, yi = verts[i]
        xj, yj = verts[j]
        if ((yi > py) != (yj > py)) and (px < (xj - xi) * (py - yi) / (yj - yi) + xi):
            cross += 1
        j = i
    return cross % 2 == 1


def py_polygon(g, untrav, trav, default, verts):
    cx = lambda i: (g.pos_x + (0.5 * g.len_x - 0.5 * g.res)) + g.res * float(-i)  # noqa: E731
    cy = lambda j: (g.pos_y + (0.5 * g.len_y - 0.5 * g.res)) + g.res * float(-j)  # noqa: E731
    xs, ys = [v[0] for v in verts], [v[1] for v in verts]
    tlx, tly = py_bound(max(xs), g.len_x, g.pos_x), py_bound(max(ys), g.len_y, g.pos_y)
    brx, bry = py_bound(min(xs), g.len_x, g.pos_x), py_bound(min(ys), g.len_y, g.pos_y)
    idx = lambda x, half, pos, n: min(max(int(-(((x - half) - pos) / g.res)), 0), n - 1)  # noqa: E731
    ti, bi = idx(tlx, 0.5 * g.len_x, g.pos_x, g.rows), idx(brx, 0.5 * g.len_x, g.pos_x, g.rows)
    tj, bj = idx(tly, 0.5 * g.len_y, g.pos_y, g.cols), idx(bry, 0.5 * g.len_y, g.pos_y, g.cols)
    n, t = 0, 0.0
    for a in range(ti, bi + 1):
        for b in range(tj, bj + 1):
            if not py_inside(verts, cx(a), cy(b)):
                continue
            o = b * g.rows + a
            if untrav[o]:
                return False, 0.0
            n += 1
            t += float(trav[o]) if np.isfinite(trav[o]) else default
    if n == 0:
        return default != 0.0, default
    return True, t / n


def untraversable_mask(oracle, g, p, elev, layers):
    _, memo = oracle.footprint(g, p, elev, layers, want_memo=True)
    return (memo["slope_footprint"] == 0) | (memo["step_footprint"] == 0) | (memo["roughness_footprint"] == 0)


def random_polygons(g, rng, count):
    """Triangles .. octagons (convex or not) around points in and around the map, some tiny, some far outside."""
    polys = []
    for k in range(count):
        cx = g.pos_x + (rng.random() - 0.5) * g.len_x * 1.3
        cy = g.pos_y + (rng.random() - 0.5) * g.len_y * 1.3
        nv = int(rng.integers(3, 9))
        scale = g.res * (0.2 if k % 7 == 0 else rng.uniform(1.5, 9.0))
        ang = np.sort(rng.random(nv)) * 2 * math.pi
        rad = scale * rng.uniform(0.4, 1.0, nv)
        polys.append(np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1))
    # cell-aligned rectangles: every edge passes through cell centres or cell borders
    for k in range(count // 4):
        i, j = int(rng.integers(0, g.rows)), int(rng.integers(0, g.cols))
        cx = (g.pos_x + (0.5 * g.len_x - 0.5 * g.res)) + g.res * float(-i)
        cy = (g.pos_y + (0.5 * g.len_y - 0.5 * g.res)) + g.res * float(-j)
        hx, hy = g.res * int(rng.integers(1, 5)) * (1.0 if k % 2 else 0.5), g.res * int(rng.integers(1, 5))
        polys.append(np.array([[cx + hx, cy + hy], [cx + hx, cy - hy], [cx - hx, cy - hy], [cx - hx, cy + hy]]))
    return polys


@pytest.mark.parametrize("shape", [(40, 31), (9, 50)])
def test_oracle_matches_python_restatement(oracle, shape):
    rows, cols = shape
    res = 0.04
    g = oracle.geom(rows, cols, res, (0.3, -1.1))
    p = oracle.default_params(fp_default=0.3)
    elev = terrain(rows, cols, seed=5)
    layers = chain_layers(oracle, g, p, elev)
    untrav = untraversable_mask(oracle, g, p, elev, layers)
    assert untrav.any() and not untrav.all()
    rng = np.random.default_rng(3)
    polys = random_polygons(g, rng, 60)
    ok, val = oracle.polygons_traversable(g, p, elev, layers["traversability_slope"], layers["traversability_step"],
                                          layers["traversability_roughness"], layers["traversability"], polys)
    n_true = 0
    for k, poly in enumerate(polys):
        want_ok, want_val = py_polygon(g, untrav, layers["traversability"], 0.3, [tuple(v) for v in poly])
        assert bool(ok[k]) == want_ok, k
        assert val[k] == want_val, (k, val[k], want_val)
        n_true += want_ok
    assert 5 < n_true < len(polys) - 5  # both outcomes are exercised
    # the footprint layers: yaw 0 turns nothing, and the layer is the per-cell polygon query
    pts = np.array(FOOTPRINT) * (res / 0.15)
    tx, trot = oracle.polygon_footprint(g, p, elev, layers["traversability_slope"], layers["traversability_step"],
                                        layers["traversability_roughness"], layers["traversability"], pts, 0.0)
    assert np.array_equal(tx.view(np.uint32), trot.view(np.uint32))
    for (i, j) in [(0, 0), (rows - 1, cols - 1), (rows // 2, cols // 3), (3, cols - 2)]:
        cx = (g.pos_x + (0.5 * g.len_x - 0.5 * g.res)) + g.res * float(-i)
        cy = (g.pos_y + (0.5 * g.len_y - 0.5 * g.res)) + g.res * float(-j)
        want_ok, want_val = py_polygon(g, untrav, layers["traversability"], 0.3, [(x + cx, y + cy) for x, y in pts])
        assert tx[j * rows + i] == np.float32(want_val if want_ok else 0.0)


def test_rotation_is_eigens_quaternion_matrix(oracle):
    """yaw -> (cos(yaw/2), 0, 0, sin(yaw/2)) -> Eigen toRotationMatrix; pi/2 is the node's default footprint_yaw."""
    pts = np.array(FOOTPRINT)
    out = oracle.rotate_footprint(pts, math.pi / 2)
    assert np.allclose(out, np.stack([-pts[:, 1], pts[:, 0]], axis=1), atol=1e-15)
    assert np.array_equal(oracle.rotate_footprint(pts, 0.0), pts)
    yaw = 0.7
    w, z = math.cos(yaw / 2), math.sin(yaw / 2)
    r00, r01 = 1.0 - (2 * z) * z, -((2 * z) * w)
    assert oracle.rotate_footprint([[1.0, 2.0]], yaw)[0, 0] == r00 * 1.0 + r01 * 2.0


# ---------------------------------------------------------------- on the device
@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import capi
    capi.load()
    return capi


def gpu_setup(capi, oracle, rows, cols, res, pos, elev, **over):
    op = oracle.default_params(**over)
    g = oracle.geom(rows, cols, res, pos)
    ctx = capi.Context(0)
    ctx.set_params(to_te_params(capi, op))
    ctx.set_geometry(rows, cols, 1, res, pos)
    ctx.upload_elevation(elev)
    ctx.run_chain(capi.RUN_FOOTPRINT)
    ctx.sync()
    layers = {k: ctx.download(k) for k in OUT_LAYERS}
    return ctx, g, op, layers


@pytest.mark.gpu
@pytest.mark.parametrize("case", EXISTING)  # (tests/polygon_cases.py: the eight footprints, each with the kernel it claims)
@pytest.mark.parametrize("per_cell", [False, True])
def test_polygon_footprint_layers(capi, oracle, case, per_cell):
    """Both kernels (offset table + LDS tile; every cell of every bounding box) against the oracle, bit for bit.  Which kernel
    a footprint takes without the option is claimed in tests/polygon_cases.py and asserted in tests/test_polygon_table.py."""
    rows, cols, res = case["rows"], case["cols"], case["res"]
    elev = terrain(rows, cols, seed=rows + cols)
    ctx, g, op, layers = gpu_setup(capi, oracle, rows, cols, res, (0.7, -0.2), elev, fp_default=0.3, **case.get("over", {}))
    with ctx:
        ctx.set_option(capi.OPT_POLYGON_PER_CELL, 1 if per_cell else 0)
        ctx.run_polygon_footprint(case["pts"], case["yaw"])
        ctx.sync()
        got_x, got_rot = ctx.download("traversability_x"), ctx.download("traversability_rot")
    # the oracle works on the layers the device produced, so this isolates the polygon pass
    want_x, want_rot = oracle.polygon_footprint(g, op, elev, layers["traversability_slope"], layers["traversability_step"],
                                                layers["traversability_roughness"], layers["traversability"],
                                                case["pts"], case["yaw"])
    assert np.array_equal(got_x.view(np.uint32), want_x.view(np.uint32)), int((got_x != want_x).sum())
    assert np.array_equal(got_rot.view(np.uint32), want_rot.view(np.uint32)), int((got_rot != want_rot).sum())
    if rows > 30 and max(abs(v) for pt in case["pts"] for v in pt) > res:
        assert (want_x == 0).any() and (want_x > 0).any()


@pytest.mark.gpu
def test_polygon_batch(capi, oracle):
    rows, cols, res = 120, 90, 0.05
    elev = terrain(rows, cols, seed=77, boxes=40)
    ctx, g, op, layers = gpu_setup(capi, oracle, rows, cols, res, (-1.0, 2.0), elev, fp_default=0.3)
    polys = random_polygons(g, np.random.default_rng(9), 400)
    with ctx:
        ok, val = ctx.polygons_traversable(polys)
        empty_ok, empty_val = ctx.polygons_traversable([])
        with pytest.raises(capi.TeError, match="no vertices"):
            ctx.polygons_traversable([polys[0], np.zeros((0, 2))])
        with pytest.raises(capi.TeError, match="not finite"):
            ctx.polygons_traversable([[[0.0, 0.0], [float("nan"), 1.0], [1.0, 1.0]]])
        with pytest.raises(capi.TeError, match="footprint points"):
            ctx.run_polygon_footprint(np.zeros((40, 2)), 0.0)
    assert len(empty_ok) == 0 and len(empty_val) == 0
    want_ok, want_val = oracle.polygons_traversable(g, op, elev, layers["traversability_slope"], layers["traversability_step"],
                                                    layers["traversability_roughness"], layers["traversability"], polys)
    assert np.array_equal(ok, want_ok)
    assert np.array_equal(val.view(np.uint64), want_val.view(np.uint64))
    assert 20 < ok.sum() < len(polys) - 20


@pytest.mark.gpu
def test_polygon_calls_need_the_mask(capi, oracle):
    rows, cols = 40, 40
    with capi.Context(0) as ctx:
        ctx.set_params(capi.default_params())
        ctx.set_geometry(rows, cols, 1, 0.05, (0.0, 0.0))
        ctx.upload_elevation(terrain(rows, cols, seed=1))
        ctx.run_chain(0)
        with pytest.raises(capi.TeError, match="footprint pass first"):
            ctx.run_polygon_footprint(FOOTPRINT, 0.0)
        with pytest.raises(capi.TeError, match="footprint pass first"):
            ctx.polygons_traversable([FOOTPRINT])
        with pytest.raises(capi.TeError):
            ctx.download("traversability_x")  # the layers do not exist before the first polygon pass
        # changing only the footprint parameters keeps the filter layers: the footprint pass alone is enough
        ctx.set_params(capi.default_params(fp_radius=0.2))
        ctx.run_footprint()
        ctx.run_polygon_footprint(FOOTPRINT, 0.0)
        ctx.sync()
        assert np.isfinite(ctx.download("traversability_x")).all()


# ---------------------------------------------------------------- polygonal footprint paths (:464-584)
def random_pose_paths(g, rng, count, scale=1.0):
    """MPC-style candidates: 1..5 poses, mostly yaw-only orientations, a few tilted, some starting outside the map."""
    paths, cons = [], []
    for k in range(count):
        n = int(rng.integers(1, 6))
        start = np.array([g.pos_x, g.pos_y]) + (rng.random(2) - 0.5) * np.array([g.len_x, g.len_y]) * (1.25 if k % 9 == 0 else 0.9)
        xy = np.vstack([start, start + np.cumsum(rng.uniform(-0.6, 0.6, size=(n - 1, 2)) * scale, axis=0)]) if n > 1 else start[None]
        yaw = rng.uniform(-math.pi, math.pi, n)
        q = np.stack([np.zeros(n), np.zeros(n), np.sin(yaw / 2), np.cos(yaw / 2)], axis=1)
        if k % 5 == 0:  # roll / pitch as well; not normalised on purpose (Eigen does not normalise either)
            q = q + rng.normal(0, 0.05, size=q.shape)
        paths.append(np.hstack([xy, rng.uniform(-0.2, 0.2, (n, 1)), q]))
        cons.append(k % 3 == 0)
    return paths, np.array(cons, np.uint8)


def py_hull(points):
    pts = [tuple(p) for p in points]
    if len(pts) <= 3:
        return pts
    s = sorted(pts)
    cw = lambda o, a, b: (a[0] - o[0]) * (b[1] - o[1]) - (b[0] - o[0]) * (a[1] - o[1]) <= 0.0  # noqa: E731
    h = []
    for p in s:
        while len(h) >= 2 and cw(h[-2], h[-1], p):
            h.pop()
        h.append(p)
    t = len(h) + 1
    for p in reversed(s[:-1]):
        while len(h) >= t and cw(h[-2], h[-1], p):
            h.pop()
        h.append(p)
    return h[:-1]


def py_area(v):
    area, j = 0.0, len(v) - 1
    for i in range(len(v)):
        area += (v[j][0] + v[i][0]) * (v[j][1] - v[i][1])
        j = i
    return abs(area / 2.0)


def py_check_polygon_path(g, untrav, trav, default, poses, points, conservative, rs=None):
    from tests.test_paths import py_inclination
    n = len(poses)
    if n == 0:
        return False, 0.0, 0.0, 2
    res_t, res_a = 0.0, 0.0
    poly2, ex, ey = [], 0.0, 0.0
    for i in range(n):
        q = [float(v) for v in poses[i]]
        poly1 = list(poly2)
        sx, sy, ex, ey = ex, ey, q[0], q[1]
        x, y, z, w = q[3:7]
        tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
        twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
        r00, r01, r02 = 1.0 - (tyy + tzz), txy - twz, txz + twy
        r10, r11, r12 = txy + twz, 1.0 - (txx + tzz), tyz - twx
        poly2 = [(((r00 * px + r01 * py) + r02 * pz) + q[0], ((r10 * px + r11 * py) + r12 * pz) + q[1]) for px, py, pz in points]
        if conservative and i > 0:
            dx, dy = ex - sx, ey - sy
            v1, v2 = list(poly1), list(poly2)
            poly2 += [(vx + dx, vy + dy) for vx, vy in v1]
            poly1 += [(vx - dx, vy - dy) for vx, vy in v2]
        if rs is not None and (n == 1 or i > 0):  # checkRobotInclination_ :526-528, :553-557
            good, outside = py_inclination(g, rs, ex, ey, ex, ey) if n == 1 else py_inclination(g, rs, sx, sy, ex, ey)
            if not good:
                return False, res_t, res_a, int(outside)
        if n == 1:
            ok, t = py_polygon(g, untrav, trav, default, poly2)
            if not ok:
                return False, res_t, res_a, 0
            res_t, res_a = t, py_area(poly2)
        if n > 1 and i > 0:
            hull = py_hull(poly1 + poly2)
            ok, t = py_polygon(g, untrav, trav, default, hull)
            if not ok:
                return False, res_t, res_a, 0
            if i > 1:
                prev, ap = res_a, py_area(hull) - py_area(poly1)
                res_a += ap
                res_t = (ap * t + prev * res_t) / res_a
            else:
                res_a, res_t = py_area(hull), t
    return True, res_t, res_a, 0


def test_oracle_polygon_paths_match_python_restatement(oracle):
    rows, cols, res = 60, 45, 0.05
    g = oracle.geom(rows, cols, res, (0.3, -1.1))
    p = oracle.default_params(fp_default=0.3)
    elev = terrain(rows, cols, seed=15, boxes=12)
    layers = chain_layers(oracle, g, p, elev)
    untrav = untraversable_mask(oracle, g, p, elev, layers)
    pts = np.array(POINTS_XYZ) * 0.5
    paths, cons = random_pose_paths(g, np.random.default_rng(21), 80, scale=0.5)
    paths.append(np.zeros((0, 7)))
    cons = np.append(cons, 0).astype(np.uint8)
    safe, val, area, st = oracle.check_polygon_paths(g, p, elev, layers["traversability_slope"], layers["traversability_step"],
                                                     layers["traversability_roughness"], layers["traversability"], paths, pts,
                                                     cons)
    for k, path in enumerate(paths):
        want = py_check_polygon_path(g, untrav, layers["traversability"], 0.3, path, [tuple(v) for v in pts], bool(cons[k]))
        assert (bool(safe[k]), val[k], area[k], int(st[k])) == want, (k, want)
    assert 10 < safe.sum() < len(paths) - 10 and st[-1] == 2


def py_path_polygons(poses, points, conservative):
    """The polygons py_check_polygon_path evaluates, with their areas."""
    out, poly2, ex, ey = [], [], 0.0, 0.0
    n = len(poses)
    for i in range(n):
        q = [float(v) for v in poses[i]]
        poly1 = list(poly2)
        sx, sy, ex, ey = ex, ey, q[0], q[1]
        x, y, z, w = q[3:7]
        tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
        twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
        r00, r01, r02 = 1.0 - (tyy + tzz), txy - twz, txz + twy
        r10, r11, r12 = txy + twz, 1.0 - (txx + tzz), tyz - twx
        poly2 = [(((r00 * px + r01 * py) + r02 * pz) + q[0], ((r10 * px + r11 * py) + r12 * pz) + q[1]) for px, py, pz in points]
        if conservative and i > 0:
            dx, dy = ex - sx, ey - sy
            v1, v2 = list(poly1), list(poly2)
            poly2 += [(vx + dx, vy + dy) for vx, vy in v1]
            poly1 += [(vx - dx, vy - dy) for vx, vy in v2]
        if n == 1:
            out.append((poly2, py_area(poly2)))
        if n > 1 and i > 0:
            hull = py_hull(poly1 + poly2)
            out.append((hull, py_area(hull)))
    return out


def test_library_path_polygons_match_python_restatement(capi):
    """te_path_polygons: the host half of the polygonal path check (pose polygons, conservative extension, monotone-chain
    hulls, areas) runs without a device; vertex for vertex and bit for bit the restatement's."""
    class G:  # only what random_pose_paths reads
        pos_x, pos_y, len_x, len_y = 0.4, -2.0, 8.0, 6.0
    paths, cons = random_pose_paths(G, np.random.default_rng(8), 300)
    # degenerate shapes: repeated poses, a two-point and a one-point "footprint"
    paths.append(np.tile(paths[0][:1], (3, 1)))
    cons = np.append(cons, 1).astype(np.uint8)
    paths.append(np.zeros((0, 7)))
    cons = np.append(cons, 0).astype(np.uint8)
    for points in (POINTS_XYZ, [[0.3, 0.0, 0.0], [-0.3, 0.1, 0.05]], [[0.0, 0.0, 0.0]],
                   [[0.3, 0.3, 0], [0.3, -0.3, 0], [0.0, -0.3, 0], [0.0, 0.0, 0], [-0.3, 0.0, 0], [-0.3, 0.3, 0]]):
        for conservative in (None, cons):
            got = capi.path_polygons(paths, points, conservative)
            assert len(got) == len(paths)
            for k, path in enumerate(paths):
                want = py_path_polygons(path, [tuple(float(v) for v in p) for p in points],
                                        bool(conservative[k]) if conservative is not None else False)
                assert len(got[k]) == len(want), k
                for (gv, ga), (wv, wa) in zip(got[k], want):
                    assert gv.shape == (len(wv), 2) and np.array_equal(gv, np.array(wv, dtype=np.float64).reshape(-1, 2)), k
                    assert ga == wa, (k, ga, wa)
    with pytest.raises(capi.TeError, match="footprint points"):
        capi.path_polygons(paths[:1], np.zeros((0, 3)))


def test_library_path_polygons_end_at_the_vertex_cap(capi):
    """A conservative path's vertex lists grow by the footprint's points with every pose.  With four points the 256th pose
    reaches kMaxPathPolygonVertices = 1024: te_path_polygons ends a longer path with the polygon of that pose, the last that
    fits -- vertex for vertex the restatement's first 255 polygons -- and gives a path of 256 poses or fewer whole."""
    t = np.arange(300)
    yaw = 0.2 + 0.002 * t
    path = np.stack([0.008 * t, 0.3 + 0.002 * t, np.zeros(300), np.zeros(300), np.zeros(300), np.sin(yaw / 2), np.cos(yaw / 2)], axis=1)
    pts = [tuple(float(v) for v in p) for p in POINTS_XYZ]
    want = py_path_polygons(path, pts, True)
    assert len(want) == 299 and len(want[254][0]) <= 2048
    got = capi.path_polygons([path, path[:256], path[:255], path], POINTS_XYZ, np.array([1, 1, 1, 0], np.uint8))
    assert [len(g) for g in got] == [255, 255, 254, 299]
    for k, n in enumerate((255, 255, 254)):
        for (gv, ga), (wv, wa) in zip(got[k], want[:n]):
            assert gv.shape == (len(wv), 2) and np.array_equal(gv, np.array(wv, dtype=np.float64).reshape(-1, 2))
            assert ga == wa
    plain = py_path_polygons(path, pts, False)  # (not conservative: four points per pose, no cap)
    for (gv, ga), (wv, wa) in zip(got[3], plain):
        assert np.array_equal(gv, np.array(wv, dtype=np.float64).reshape(-1, 2)) and ga == wa


@pytest.mark.gpu
def test_polygon_paths_on_the_device(capi, oracle):
    rows, cols, res = 160, 140, 0.05
    elev = terrain(rows, cols, seed=31, boxes=12)
    ctx, g, op, layers = gpu_setup(capi, oracle, rows, cols, res, (2.0, -3.0), elev, fp_default=0.3)
    paths, cons = random_pose_paths(g, np.random.default_rng(4), 5000)  # >= 4096: the host side builds the polygons on several threads
    paths.append(np.zeros((0, 7)))
    cons = np.append(cons, 1).astype(np.uint8)
    with ctx:
        got = ctx.check_polygon_footprint_paths(paths, POINTS_XYZ, cons)
        got_nc = ctx.check_polygon_footprint_paths(paths, POINTS_XYZ)
        assert all(len(v) == 0 for v in ctx.check_polygon_footprint_paths([], POINTS_XYZ))
        with pytest.raises(capi.TeError, match="footprint points"):
            ctx.check_polygon_footprint_paths(paths[:1], np.zeros((0, 3)))
        with pytest.raises(capi.TeError, match="not finite"):
            ctx.check_polygon_footprint_paths([np.full((2, 7), np.nan)], POINTS_XYZ)
    args = (g, op, elev, layers["traversability_slope"], layers["traversability_step"], layers["traversability_roughness"],
            layers["traversability"], paths, POINTS_XYZ)
    for have, want in ((got, oracle.check_polygon_paths(*args, cons)), (got_nc, oracle.check_polygon_paths(*args))):
        assert np.array_equal(have[0], want[0]) and np.array_equal(have[3], want[3])
        assert np.array_equal(have[1].view(np.uint64), want[1].view(np.uint64))
        assert np.array_equal(have[2].view(np.uint64), want[2].view(np.uint64))
    assert 50 < got[0].sum() < len(paths) - 50
    assert not np.array_equal(got[0], got_nc[0]) or not np.array_equal(got[2], got_nc[2])  # conservative matters
