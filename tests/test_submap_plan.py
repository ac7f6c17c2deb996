"""The geometry of a submap request (traversability_estimation_amd/csrc/te_submap_plan.h, handed out by te_submap_geometry)
against the independent restatement of GridMap::getSubmap in tests/ref_py/grid_map_ref.py: field for field, the doubles bit
for bit.  tests/cpu/submap_plan_check.cpp is the same header as a stand-alone program, run plain and under the sanitizers."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.ref_py.grid_map_ref import GridMapRef

SRC = os.path.join(ROOT, "tests", "cpu", "submap_plan_check.cpp")
INC = [os.path.join(ROOT, "traversability_estimation_amd", "csrc"), os.path.join(ROOT, "include")]

MAPS = [(1, 1), (7, 5), (37, 29), (100, 133)]
RESOLUTIONS = [0.03, 0.05, 0.1]
POSITIONS = [(0.0, 0.0), (100.0, -250.3), (-3.25, 7.5)]
N_REQUESTS = 2000


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    return capi


def bits(x):
    return struct.pack("<d", x)


def assert_same(capi, shape, res, pos, centre, length):
    """te_submap_geometry against GridMapRef.submap for one request; returns ok."""
    gm = GridMapRef(shape[0], shape[1], res, pos)
    ok, tl, size, sub = gm.submap(centre, length)
    got = capi.submap_geometry(shape[0], shape[1], res, pos, centre, length)
    what = f"{shape} at {res} around {pos}: request {centre!r} + {length!r}"
    assert bool(got.ok) == ok, what
    if not ok:
        assert (got.row0, got.col0, got.rows, got.cols) == (0, 0, 0, 0), what
        assert (got.pos_x, got.pos_y, got.length_x, got.length_y) == (0.0, 0.0, 0.0, 0.0), what
        return False
    assert (got.row0, got.col0) == tl and (got.rows, got.cols) == size, (what, got.row0, got.col0, got.rows, got.cols, tl, size)
    for mine, theirs in ((got.pos_x, sub.pos[0]), (got.pos_y, sub.pos[1]), (got.length_x, sub.length[0]), (got.length_y, sub.length[1])):
        assert bits(mine) == bits(theirs), (what, mine, theirs)
    return True


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_submap_plan_program(tmp_path, flags):
    exe = str(tmp_path / "submap_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + [a for d in INC for a in ("-I", d)] + [SRC, "-o", exe], check=True,
                   timeout=300)
    for seed in (1, 2):
        r = subprocess.run([exe, "4000", str(seed)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
        assert "4000 random requests" in r.stdout and ", 0 failed checks" in r.stdout


def random_requests():
    """2 000 seeded requests: (shape, resolution, map position, centre, length).  Centres uniform in the map's extent widened by
    10 % on every side, lengths from 0 to 1.5 x the map's (one in 16 exactly 0)."""
    rng = np.random.default_rng(20240607)
    out = []
    for k in range(N_REQUESTS):
        shape = MAPS[k % len(MAPS)]
        res = RESOLUTIONS[(k // len(MAPS)) % len(RESOLUTIONS)]
        pos = POSITIONS[int(rng.integers(len(POSITIONS)))]
        ext = (shape[0] * res, shape[1] * res)
        centre = tuple(float(pos[a] + (rng.random() - 0.5) * 1.2 * ext[a]) for a in (0, 1))
        length = tuple(0.0 if rng.integers(16) == 0 else float(rng.random() * 1.5 * ext[a]) for a in (0, 1))
        out.append((shape, res, pos, centre, length))
    return out


def test_random_requests_bit_for_bit(capi):
    reqs = random_requests()
    # on the restatement alone: the sweep reaches both outcomes (a centre inside the map is ok: (1 / 1.2)^2 = 69 % of the draws)
    oks = [GridMapRef(s[0], s[1], res, pos).submap(c, ln)[0] for s, res, pos, c, ln in reqs]
    assert sum(oks) >= N_REQUESTS // 2 and len(oks) - sum(oks) >= 50, (sum(oks), len(oks))
    assert any(p == (100.0, -250.3) for _, _, p, _, _ in reqs)
    n_ok = sum(assert_same(capi, *r) for r in reqs)
    assert n_ok == sum(oks)


@pytest.mark.parametrize("shape", MAPS)
@pytest.mark.parametrize("res", RESOLUTIONS)
def test_named_requests(capi, shape, res):
    pos = (100.0, -250.3)
    ext = (shape[0] * res, shape[1] * res)
    # the whole map, and a request larger than the map (clamped to it)
    for f in (1.0, 1.3, 50.0):
        assert assert_same(capi, shape, res, pos, pos, (f * ext[0], f * ext[1]))
        got = capi.submap_geometry(shape[0], shape[1], res, pos, pos, (f * ext[0], f * ext[1]))
        assert (got.row0, got.col0, got.rows, got.cols) == (0, 0, shape[0], shape[1])
    # zero length: one cell; the far corner cell; a length on one axis only
    gm = GridMapRef(shape[0], shape[1], res, pos)
    for cell in ((0, 0), (shape[0] - 1, shape[1] - 1), (shape[0] // 2, shape[1] // 3)):
        c = gm.position(cell)
        assert assert_same(capi, shape, res, pos, c, (0.0, 0.0))
        got = capi.submap_geometry(shape[0], shape[1], res, pos, c, (0.0, 0.0))
        assert (got.row0, got.col0, got.rows, got.cols) == (cell[0], cell[1], 1, 1)
        assert_same(capi, shape, res, pos, c, (2.5 * res, 2.5 * res))
        assert_same(capi, shape, res, pos, c, (0.0, 10 * res))
    # the centre exactly on each of the four borders (the two outcomes are the restatement's)
    for length in ((0.0, 0.0), (2.5 * res, 2.5 * res), (ext[0], ext[1])):
        for centre in ((pos[0] + 0.5 * ext[0], pos[1]), (pos[0] - 0.5 * ext[0], pos[1]), (pos[0], pos[1] + 0.5 * ext[1]),
                       (pos[0], pos[1] - 0.5 * ext[1]), (pos[0] + 0.5 * ext[0], pos[1] - 0.5 * ext[1])):
            assert_same(capi, shape, res, pos, centre, length)
    # well outside
    assert not assert_same(capi, shape, res, pos, (pos[0] + 2 * ext[0], pos[1]), (res, res))


def test_arguments_are_checked_before_anything_is_computed(capi):
    for bad in (math.nan, math.inf, -math.inf):
        for centre, length in (((bad, 0.0), (1.0, 1.0)), ((0.0, bad), (1.0, 1.0)), ((0.0, 0.0), (bad, 1.0)), ((0.0, 0.0), (1.0, bad))):
            with pytest.raises(capi.TeError) as e:
                capi.submap_geometry(10, 10, 0.1, (0.0, 0.0), centre, length)
            assert e.value.code == capi.TE_ERR_INVALID_ARG and "te_submap_geometry" in str(e.value)
    for length in ((-1e-12, 1.0), (1.0, -3.0)):
        with pytest.raises(capi.TeError) as e:
            capi.submap_geometry(10, 10, 0.1, (0.0, 0.0), (0.0, 0.0), length)
        assert e.value.code == capi.TE_ERR_INVALID_ARG and "negative" in str(e.value)
    for rows, cols, res, pos in ((0, 10, 0.1, (0.0, 0.0)), (10, -1, 0.1, (0.0, 0.0)), (10, 10, 0.0, (0.0, 0.0)), (10, 10, math.nan, (0.0, 0.0)),
                                 (10, 10, 0.1, (math.inf, 0.0))):
        with pytest.raises(capi.TeError) as e:
            capi.submap_geometry(rows, cols, res, pos, (0.0, 0.0), (1.0, 1.0))
        assert e.value.code == capi.TE_ERR_INVALID_ARG
    assert capi.load().te_submap_geometry(10, 10, 0.1, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, None) == capi.TE_ERR_INVALID_ARG
    # zero and minus zero are valid lengths
    assert capi.submap_geometry(10, 10, 0.1, (0.0, 0.0), (0.01, 0.01), (-0.0, 0.0)).ok == 1
