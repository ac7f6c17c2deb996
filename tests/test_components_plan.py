"""The routines of te_run_components / te_run_reachable (csrc/te_components.h) and their plan (csrc/te_components_plan.h) on the
CPU: tests/cpu/components_check.cpp labels every binary map up to 4 x 4 with the headers' own routines, tile by tile with tile
edges forced down to 2 and 3 cells, against a flood fill; checks the run extraction against a bit loop; and checks that every
cell has one owning tile and every seam cell is visited once -- plain and, as a stand-alone program, under the sanitizers.  And
the shapes of tests/components_cases.py have the tiles their GPU test relies on, with the designed inputs crossing the seams;
which shapes make the write pass take a second turn (BIG, BIG_THIN, FLOAT_INEXACT) and which cannot (every one of SHAPES); and
the seam cells of `islands` and `perforated` are where their GPU tests need them."""
import os
import subprocess

import numpy as np
import pytest

from tests import components_cases as K
from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpu", "components_check.cpp")
INC = os.path.join(ROOT, "traversability_estimation_amd", "csrc")


def build(tmp, flags):
    exe = str(tmp / "components_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", INC, SRC, "-o", exe], check=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("components_plan"), ["-O2"])


def out(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout.strip()


def test_check_program(exe):
    assert ", 0 failed checks" in out(exe)


def test_check_program_under_the_sanitizers(tmp_path):
    assert ", 0 failed checks" in out(build(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


def tiles(exe, rows, cols):
    f = out(exe, "tiles", rows, cols).split()
    return dict(tiles_i=int(f[0]), tiles_j=int(f[1]), ti=int(f[2]), tj=int(f[3]), seam_cells=int(f[4]), scratch=int(f[5]), fits=f[6] == "1",
                flat_blocks=int(f[7]), write_blocks=int(f[8]))


@pytest.mark.parametrize("rows,cols", K.SHAPES)
def test_gpu_shapes_have_the_tiles_they_claim(exe, rows, cols):
    t = tiles(exe, rows, cols)
    assert (t["tiles_i"], t["tiles_j"]) == (-(-rows // t["ti"]), -(-cols // t["tj"])) and t["fits"]
    assert t["scratch"] == 8 * rows * cols  # the contract: at most 8 bytes per cell of the call
    assert t["seam_cells"] == (t["tiles_j"] - 1) * rows + (t["tiles_i"] - 1) * cols
    if (rows, cols) in K.MULTI_TILE:
        want_i, want_j = K.MULTI_TILE[(rows, cols)]
        assert t["tiles_i"] >= want_i and t["tiles_j"] >= want_j
    else:
        assert (t["tiles_i"], t["tiles_j"]) == (1, 1)


def crossings(free, ti, tj, di, dj):
    """(pairs of free cells (i, j), (i + di, j + dj) that straddle a column seam, a row seam)"""
    rows, cols = free.shape
    i, j = np.indices((rows, cols))
    p, q = i + di, j + dj
    ok = (p >= 0) & (p < rows) & (q >= 0) & (q < cols)
    both = np.zeros_like(free)
    both[ok] = free[ok] & free[p[ok], q[ok]]
    over_col = both & ok & (j // tj != np.clip(q, 0, cols - 1) // tj)
    over_row = both & ok & (i // ti != np.clip(p, 0, rows - 1) // ti)
    return int(over_col.sum()), int(over_row.sum())


@pytest.mark.parametrize("rows,cols", K.BOTH_SEAMS)
def test_designed_inputs_cross_a_seam_in_both_directions(exe, rows, cols):
    t = tiles(exe, rows, cols)
    assert t["tiles_i"] >= 2 and t["tiles_j"] >= 2
    m = K.masks(rows, cols, 1)
    for name in ("spiral", "comb", "two_combs"):
        over_col, _ = crossings(m[name][0], t["ti"], t["tj"], 0, 1)
        _, over_row = crossings(m[name][0], t["ti"], t["tj"], 1, 0)
        assert over_col > 0 and over_row > 0, name
    # the diagonal crosses both kinds of seam by diagonal steps alone; at a tile corner one step crosses both at once
    over_col, over_row = crossings(m["diagonal"][0], t["ti"], t["tj"], 1, 1)
    assert over_col > 0 and over_row > 0
    assert crossings(m["diagonal"][0], t["ti"], t["tj"], 0, 1) == (0, 0) and crossings(m["diagonal"][0], t["ti"], t["tj"], 1, 0) == (0, 0)
    # the two combs touch by one diagonal step and by no straight one (tests/test_components_ref.py counts the components)
    assert len(K.BOTH_SEAMS) >= 3


@pytest.mark.parametrize("rows,cols", K.SHAPES)
def test_the_write_pass_takes_one_turn_on_every_shape_of_the_sweep(exe, rows, cols):
    """What the sweep over SHAPES cannot reach: a thread of the write pass that takes a second cell."""
    t = tiles(exe, rows, cols)
    assert t["flat_blocks"] == t["write_blocks"] == -(-rows * cols // 256)
    assert rows * cols <= K.WRITE_TURN


@pytest.mark.parametrize("rows,cols", [K.BIG, K.BIG_THIN, K.FLOAT_INEXACT])
def test_the_large_shapes_make_the_write_pass_take_a_second_turn(exe, rows, cols):
    t = tiles(exe, rows, cols)
    assert t["flat_blocks"] > t["write_blocks"] == 4096 and t["fits"]
    assert t["write_blocks"] * 256 == K.WRITE_TURN < rows * cols
    if (rows, cols) == K.BIG:  # some threads take a second turn and most do not
        assert rows * cols - K.WRITE_TURN == 7424
    if (rows, cols) == K.BIG_THIN:
        assert (t["tiles_i"], t["tiles_j"]) == (257, 2) and rows * cols < 2 * K.WRITE_TURN
    if (rows, cols) == K.FLOAT_INEXACT:  # the smallest square map whose cell count float32 rounds
        n = rows * cols
        assert n > 2 ** 24 and int(np.float32(np.uint32(n))) != n and int(np.float32(np.uint32((rows - 1) * (cols - 1)))) == (rows - 1) * (cols - 1)


def test_islands_straddle_a_seam_of_each_kind(exe):
    rows, cols = K.ISLANDS_SHAPE
    t = tiles(exe, rows, cols)
    f = K.islands(rows, cols)
    over_col, _ = crossings(f, t["ti"], t["tj"], 0, 1)
    _, over_row = crossings(f, t["ti"], t["tj"], 1, 0)
    # block row 21 is rows 63 and 64, block column 21 is columns 63 and 64: two straight steps of every such island cross
    na, nb = K.island_grid(rows, cols)
    assert over_col == 2 * na and over_row == 2 * nb
    assert f[63:65, 63:65].all()  # one island lies on the tile corner


@pytest.mark.parametrize("rows,cols", K.PERFORATED_SHAPES)
@pytest.mark.parametrize("split", [False, True])
def test_perforated_seams_save_no_union_and_many_threads_share_two_roots(exe, rows, cols, split):
    t = tiles(exe, rows, cols)
    ti, tj = t["ti"], t["tj"]
    assert t["tiles_i"] >= 4 and t["tiles_j"] >= 4
    f = K.perforated(rows, cols, split)
    # every free cell on a seam has a blocked cell before it along that seam (the first cell of a seam has none before it):
    # seam_col_cell / seam_row_cell then issue their straight union at every one of them
    for j in range(tj, cols, tj):
        assert not (f[1:, j] & f[:-1, j]).any() and not f[1::2, j].any()
    for i in range(ti, rows, ti):
        assert not (f[i, 1:] & f[i, :-1]).any() and not f[i, 1::2].any()
    # per tile edge of n cells, at least n // 2 - 2 free seam cells face a free cell across the seam: 30 on a whole edge of 64
    edges = 0
    for j in range(tj, cols, tj):
        for i0 in range(0, rows, ti):
            facing = f[i0:i0 + ti, j] & f[i0:i0 + ti, j - 1]
            assert int(facing.sum()) >= min(ti, rows - i0) // 2 - 2
            edges += min(ti, rows - i0) == 64
    for i in range(ti, rows, ti):
        for j0 in range(0, cols, tj):
            facing = f[i, j0:j0 + tj] & f[i - 1, j0:j0 + tj]
            assert int(facing.sum()) >= min(tj, cols - j0) // 2 - 2
            edges += min(tj, cols - j0) == 64
    assert edges >= 18 and 64 // 2 - 2 == 30
