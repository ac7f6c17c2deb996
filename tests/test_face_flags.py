"""The face flags of an elevation layer (traversability_estimation_amd/csrc/te_face_flags.h): one byte per 64 x 4 cells, 1 iff
some in-map cell within Chebyshev distance 2 of the granule lies more than fp_critical_step above the NaN-ignoring minimum of
its 3x3 block.  tests/cpu/face_flags_check.cpp is compiled from the header the library itself uses; it checks every tile of
the mask kernel (MY = 4, 8, 32) -- a tile with a lower step neighbour has a flag set, and with step scores of 0 throughout
exactly those tiles have -- and writes the flags, which are compared here with a numpy restatement of the definition."""
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

GI, GJ, DIL = 64, 4, 2


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("face")
    exe = d / "face_flags_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "traversability_estimation_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpu", "face_flags_check.cpp"), "-o", str(exe)], check=True, timeout=300)

    def run(elev, step, crit):
        """elev, step: (batch, cols, rows) float32 (cell (i, j) at [j, i], the device's memory order).  Returns (flags
        (batch, nfy, ntx), hit' (batch, cols, rows)) as the header computes them; fails if a tile check does."""
        elev = np.ascontiguousarray(elev, np.float32)
        step = np.ascontiguousarray(step, np.float32)
        batch, cols, rows = elev.shape
        fin, fout = d / "in.bin", d / "out.bin"
        with open(fin, "wb") as f:
            f.write(elev.tobytes())
            f.write(step.tobytes())
        r = subprocess.run([str(exe), str(rows), str(cols), str(batch), repr(float(crit)), str(fin), str(fout)], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        raw = np.fromfile(fout, np.uint8)
        ntx, nfy = (rows + GI - 1) // GI, (cols + GJ - 1) // GJ
        nf = batch * nfy * ntx
        assert raw.size == nf + elev.size
        return raw[:nf].reshape(batch, nfy, ntx), raw[nf:].reshape(batch, cols, rows)
    return run


def flags_numpy(elev, crit):
    """The definition, restated: hit' per cell, dilated by 2 cells within the map, reduced per granule."""
    elev = np.asarray(elev, np.float32)
    batch, cols, rows = elev.shape
    pad = np.full((batch, cols + 2, rows + 2), np.nan, np.float32)
    pad[:, 1:-1, 1:-1] = elev
    mn = np.full_like(elev, np.nan)
    for dj in range(3):
        for di in range(3):
            mn = np.fmin(mn, pad[:, dj:dj + cols, di:di + rows])  # (fmin ignores NaN)
    with np.errstate(invalid="ignore"):
        hit = mn.astype(np.float64) < elev.astype(np.float64) - float(crit)
    wide = np.zeros((batch, cols + 2 * DIL, rows + 2 * DIL), bool)
    for dj in range(2 * DIL + 1):
        for di in range(2 * DIL + 1):
            wide[:, dj:dj + cols, di:di + rows] |= hit
    near = wide[:, DIL:-DIL, DIL:-DIL]  # some hit' cell within 2 cells
    ntx, nfy = (rows + GI - 1) // GI, (cols + GJ - 1) // GJ
    full = np.zeros((batch, nfy * GJ, ntx * GI), bool)
    full[:, :cols, :rows] = near
    return full.reshape(batch, nfy, GJ, ntx, GI).any(axis=(2, 4)).astype(np.uint8), hit.astype(np.uint8)


def terrain(rng, rows, cols):
    """Smooth ground (adjacent cells differ by millimetres) with NaN speckle, NaN regions, plateaus and single-cell spikes."""
    j, i = np.meshgrid(np.arange(cols), np.arange(rows), indexing="ij")
    e = (0.05 * np.sin(i / 17.0) + 0.04 * np.cos(j / 11.0) + 0.002 * rng.standard_normal((cols, rows))).astype(np.float32)
    for _ in range(int(rng.integers(0, 4))):  # plateaus: faces along their edges
        a, b = int(rng.integers(0, rows)), int(rng.integers(0, cols))
        e[b:b + int(rng.integers(1, 40)), a:a + int(rng.integers(1, 40))] += np.float32(rng.choice([-0.3, 0.13, 0.3]))
    for _ in range(int(rng.integers(0, 5))):  # spikes
        e[int(rng.integers(0, cols)), int(rng.integers(0, rows))] += np.float32(rng.choice([0.5, -0.5, np.inf]))
    e[rng.random((cols, rows)) < 0.01] = np.nan
    if rng.random() < 0.5:
        a, b = int(rng.integers(0, rows)), int(rng.integers(0, cols))
        e[b:b + 20, a:a + 30] = np.nan
    return e


@pytest.mark.parametrize("seed", range(12))
def test_random_maps_sound_for_every_tile_and_equal_to_the_definition(checker, seed):
    rng = np.random.default_rng(4100 + seed)
    rows = [200, 64, 65, 127, 193, 1, 3][seed % 7]  # (rows not a multiple of 64 ...)
    cols = [150, 4, 5, 33, 150, 7, 2][seed % 7]     # (... columns not a multiple of 4)
    batch = 2 if seed % 5 == 4 else 1
    elev = np.stack([terrain(rng, rows, cols) for _ in range(batch)])
    step_kind = seed % 3  # step == 0 nowhere, everywhere, random
    step = [np.ones_like(elev), np.zeros_like(elev), (rng.random(elev.shape) < 0.5).astype(np.float32)][step_kind]
    step[rng.random(elev.shape) < 0.02] = np.nan
    crit = [0.12, 0.03, 0.0, 0.25][seed % 4]
    flags, hit = checker(elev, step, crit)
    want_flags, want_hit = flags_numpy(elev, crit)
    assert np.array_equal(hit, want_hit)
    assert np.array_equal(flags, want_flags)


def test_all_nan_and_flat_maps_have_no_flag(checker):
    for e in (np.full((1, 70, 130), np.nan, np.float32), np.zeros((1, 70, 130), np.float32)):
        flags, hit = checker(e, np.zeros_like(e), 0.12)
        assert not flags.any() and not hit.any()


def test_a_drop_of_exactly_the_critical_step_and_one_ulp_either_side(checker):
    """hit' is  (double)min < (double)elev - crit  -- strict, in double: a cell exactly crit above its lowest neighbour is no face."""
    crit = 0.125  # (a float32 and a double alike)
    for base in (0.0, 1.0, -3.5):
        top = np.float32(base) + np.float32(crit)
        assert float(top) - float(np.float32(base)) == crit
        for value, want in ((top, 0), (np.nextafter(top, np.float32(np.inf)), 1), (np.nextafter(top, np.float32(-np.inf)), 0)):
            e = np.full((1, 40, 100), base, np.float32)
            e[0, 20, 50] = value
            flags, hit = checker(e, np.zeros_like(e), crit)
            assert int(hit.sum()) == want and int(hit[0, 20, 50]) == want
            assert bool(flags.any()) == bool(want)
    # crit = 0.12 is no float32: float32(0.12) < 0.12 < its successor
    e = np.zeros((1, 40, 100), np.float32)
    e[0, 20, 50] = np.float32(0.12)
    assert not checker(e, np.zeros_like(e), 0.12)[0].any()
    e[0, 20, 50] = np.nextafter(np.float32(0.12), np.float32(1.0))
    assert checker(e, np.zeros_like(e), 0.12)[0].any()


def granule_distance(i, j, gi, gj, rows, cols):
    """Chebyshev distance of cell (i, j) from the in-map cells of granule (gi, gj)."""
    i_lo, i_hi = gi * GI, min(gi * GI + GI, rows) - 1
    j_lo, j_hi = gj * GJ, min(gj * GJ + GJ, cols) - 1
    return max(max(i_lo - i, 0, i - i_hi), max(j_lo - j, 0, j - j_hi))


def test_a_single_face_cell_sets_the_granules_within_two_cells(checker):
    """One spike (hit' in exactly its own cell) at distance 0 .. 3 from granule and tile borders in i (the 64-cell granule
    columns), in j (the 4-cell granule rows, the tile rows of MY = 8 and 32) and diagonally; on a map whose last granules are
    partial (rows no multiple of 64, columns no multiple of 4)."""
    rows, cols = 200, 70
    spots = []
    for d in range(4):
        spots += [(64 + d, 17), (63 - d, 17), (128 + d, 33), (127 - d, 33)]      # across i = 64 k
        spots += [(30, 32 + d), (30, 31 - d), (100, 8 + d), (100, 7 - d)]       # across the tile rows j = 32, 8
        spots += [(64 + d, 32 + d), (63 - d, 31 - d), (64 + d, 31 - d), (127 - d, 8 + d)]  # diagonally, at tile corners
        spots += [(d, d), (rows - 1 - d, cols - 1 - d), (192 + d, 68), (199, 64 + d)]     # map corners, the partial granules
    for i, j in spots:
        e = np.zeros((1, cols, rows), np.float32)
        e[0, j, i] = 1.0
        flags, hit = checker(e, np.ones_like(e), 0.12)  # (no step score is 0: the flags do not look at the scores)
        assert int(hit.sum()) == 1 and hit[0, j, i] == 1
        for gj in range(flags.shape[1]):
            for gi in range(flags.shape[2]):
                assert int(flags[0, gj, gi]) == (1 if granule_distance(i, j, gi, gj, rows, cols) <= DIL else 0), (i, j, gi, gj)
