"""te_fp_table.h on the CPU, from the header the route of any reach is built from (te_footprint_any.hip): for footprints of
21 to 150 cells its spiral is the oracle's SpiralIterator (order, ring distances; the tie-flagged entries exactly the ones
isInside decides per centre), its runs and ties are the same disc, and the clip to the map drops exactly the offsets no
centre of the map can reach.  Up to a reach of 20 cells the kernels read the same spiral packed into one word per entry."""
import math
import os
import subprocess

import pytest

from tests.conftest import ROOT

# (rmax in cells, what the case exercises): whole-cell radii are tie radii
RADII = [(21.3, "reach 21"), (22.5, "the default YAML at 0.02 m"), (23.3, "reach 23"), (25.0, "ties 7-24-25, 15-20-25"),
         (45.0, "the default YAML at 0.01 m"), (65.0, "36 ties"), (150.3, "reach 150")]
RES = (0.01, 0.02, 0.03)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("fp_table") / "fp_table_check"
    src = os.path.join(ROOT, "tests", "cpu", "fp_table_check.cpp")
    inc = os.path.join(ROOT, "traversability_estimation_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", inc, src, "-o", str(out)], check=True,
                   timeout=300)
    return str(out)


def table(exe, rmax, res, rows, cols, clip):
    r = subprocess.run([exe, repr(rmax), repr(res), str(rows), str(cols), "1" if clip else "0"], capture_output=True, text=True,
                       timeout=120, check=True)
    lines = r.stdout.split("\n")
    reach, R, n_runs, n_ties, n_spiral, n_full = (int(v) for v in lines[0].split())
    hw = [int(v) for v in lines[1].split()]
    tv = [int(v) for v in lines[2].split()]
    ties = list(zip(tv[0::2], tv[1::2]))
    spiral = [tuple(int(v) for v in ln.split()) for ln in lines[3:3 + n_spiral]]
    assert len(hw) == n_runs and len(ties) == n_ties and len(spiral) == n_spiral
    return dict(reach=reach, R=R, hw=hw, ties=ties, spiral=spiral, n_full=n_full)


def walk_matches(entries, want, ctx):
    """entries: the table filtered to one centre's map cells; want: the oracle's (di, dj, ring) in visiting order.  A tie
    entry the oracle does not visit was rejected by isInside; every other entry must be visited, in the same order."""
    k = 0
    for di, dj, ring, tie in entries:
        if k < len(want) and (di, dj) == want[k][:2]:
            assert ring == want[k][2], (ctx, k, di, dj, ring, want[k])
            k += 1
        else:
            assert tie, (ctx, "entry not visited by the oracle", k, (di, dj, ring), want[k] if k < len(want) else None)
    assert k == len(want), (ctx, "the oracle visits more cells", k, len(want))


@pytest.mark.parametrize("cells,what", RADII, ids=[w for _, w in RADII])
def test_spiral_runs_and_ties(exe, cells, what):
    for res in RES:
        rmax = cells * res
        full = table(exe, rmax, res, 1, 1, clip=False)
        q = (rmax / res) ** 2
        tol = 1e-9 * max(q, 1.0)
        sp = full["spiral"]
        assert full["n_full"] == len(sp)
        assert sp[0] == (0, 0, 0, 0)
        nrings = math.ceil(rmax / res)
        seen = set()
        for di, dj, ring, tie in sp:
            m = di * di + dj * dj
            assert ring == int(math.sqrt(m)), (di, dj, ring)
            assert tie == (1 if abs(m - q) <= tol and ring >= nrings - 1 else 0), (res, di, dj, tie)
            assert (di, dj) not in seen
            seen.add((di, dj))
        # rings in order, each ring whole
        rings = [e[2] for e in sp]
        assert rings == sorted(rings)
        # the runs and ties name the same disc as the spiral
        runs = {(di, dj) for dj in range(-full["R"], full["R"] + 1) for di in range(-full["hw"][abs(dj)], full["hw"][abs(dj)] + 1)}
        assert runs == {(e[0], e[1]) for e in sp if not e[3]}, (what, res)
        assert set(full["ties"]) == {(e[0], e[1]) for e in sp if e[3]}, (what, res)
        assert full["reach"] == max(max(abs(e[0]), abs(e[1])) for e in sp)
        if cells == 65.0:
            assert len(full["ties"]) == 36
        if cells == 25.0:
            assert len(full["ties"]) == 20  # (+-25, 0), (0, +-25), (+-7, +-24), (+-24, +-7), (+-15, +-20), (+-20, +-15)


@pytest.mark.parametrize("cells,what", RADII, ids=[w for _, w in RADII])
def test_clip_and_oracle_walk(exe, oracle, cells, what):
    for res, (rows, cols), pos in ((0.01, (70, 50), (0.0, 0.0)), (0.02, (64, 48), (1.37, -2.11)), (0.03, (130, 97), (-5.5, 3.25)),
                                   (0.02, (301, 257), (0.003, 0.007))):
        rmax = cells * res
        full = table(exe, rmax, res, rows, cols, clip=False)
        clipped = table(exe, rmax, res, rows, cols, clip=True)
        keep = [e for e in full["spiral"] if abs(e[0]) < rows and abs(e[1]) < cols]
        assert clipped["spiral"] == keep, (what, res, rows, cols)
        assert clipped["n_full"] == len(full["spiral"])
        assert len(clipped["spiral"]) <= (2 * rows - 1) * (2 * cols - 1)
        assert clipped["ties"] == [t for t in full["ties"] if abs(t[0]) < rows and abs(t[1]) < cols]
        assert clipped["R"] == min(full["R"], cols - 1)
        assert clipped["hw"] == [min(h, rows - 1) for h in full["hw"][:clipped["R"] + 1]]
        g = oracle.geom(rows, cols, res, pos)
        centres = {(0, 0), (rows - 1, cols - 1), (0, cols - 1), (rows - 1, 0), (rows // 2, cols // 2), (1, cols // 3),
                   (rows // 3, 0), (rows - 2, cols - 3)}
        for ci, cj in sorted(centres):
            di, dj, rg = oracle.spiral_offsets(g, ci, cj, rmax, cap=400000)
            want = list(zip(di.tolist(), dj.tolist(), rg.tolist()))
            mine = [e for e in clipped["spiral"] if 0 <= ci + e[0] < rows and 0 <= cj + e[1] < cols]
            walk_matches(mine, want, (what, res, rows, cols, ci, cj))


# reach <= 20: the packed words the kernels of those reaches read (fp_pack); whole-cell and Pythagorean tie radii included
PACKED = [0.5, 1.0, 1.5, 2.0, 2.9, 5.0, 6.3, 9.000009, 10.0, 12.5, 13.0, 15.0, 16.000016, 17.0, 18.5, 19.7, 20.0, 20.99]


@pytest.mark.parametrize("cells", PACKED)
def test_packed_spiral_round_trips(exe, cells):
    for res in RES:
        n, reach, bad = (int(v) for v in subprocess.run([exe, "pack", repr(cells * res), repr(res)], capture_output=True, text=True,
                                                         timeout=120, check=True).stdout.split())
        assert reach <= 20 and bad == 0, (cells, res, reach, bad)
        assert n == table(exe, cells * res, res, 1, 1, clip=False)["n_full"]
        if cells in (5.0, 10.0, 13.0, 15.0, 17.0, 20.0):  # ties with both parts non-zero: the tie flag round-trips too
            assert sum(e[3] for e in table(exe, cells * res, res, 1, 1, clip=False)["spiral"]) == 12
