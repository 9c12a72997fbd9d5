"""The cases of tests/gso_shapes.py on the oracle alone (no GPU): the launch arithmetic each row claims, the paths the swarms
reach, and how far the reference's own decisions are from a knife edge -- what tests/test_gpu_gso_shapes.py then holds the
kernels to would otherwise depend on a rounding.

Margins, at every step of every replayed swarm, from the positions and vision ranges before the step and the luciferins after
its update (the ones the neighbour search compares):
  * over all pairs (i, j) with distance d < vr_i + 1e-6 and non-identical poses, |l_i - l_j| >= 1e-7: the GPU's luciferins are
    held to 1e-9 relative, about 5e-9 absolute, so `l_i < l_j` cannot come out differently;
  * over all pairs with l_j > l_i, |d - vr_i| >= 1e-9: the GPU's poses are held to 1e-12, so `d < vr_i` cannot either.
The roulette's margin |sum - rnd| is not checked: the oracle does not expose the draw.
"""
import numpy as np
import pytest

import gso_shapes
from gso_shapes import CASES, B3_THIRD_TRIP, K2_ALL, launch, sampled_swarms

MIN_LUCIFERIN_GAP = 1e-7
MIN_RANGE_GAP = 1e-9
LINEAR_THRESHOLD = 0.9995    # src/constants.rs:11


@pytest.fixture(scope="module")
def shapes(pkg, orc, table, tmp_path_factory):
    return gso_shapes.shapes(pkg, orc, table, str(tmp_path_factory.mktemp("gso_shapes")))


def test_case_table_is_complete():
    assert sorted(CASES) == ["A1", "A2", "A3", "A4", "A5", "B1", "B2", "B3", "C1", "C2", "C3"]
    for name, c in CASES.items():
        assert set(c["expect"]) == set(c["k2"]), name
        assert c["N"] <= gso_shapes.MAX_GLOWWORMS
        if c["modes"]:
            assert max(c["modes"]) <= 64


@pytest.mark.parametrize("case", sorted(CASES))
def test_launch_arithmetic_of_the_table(case):
    """Every figure a row spells out is what the restated launch formulas give."""
    c = CASES[case]
    for k2 in c["k2"]:
        got = launch(c["S"], c["N"], k2)
        for key, want in c["expect"][k2].items():
            assert got[key] == want, (case, k2, key, got[key], want)
        assert got["lds"] <= gso_shapes.LDS_LIMIT
        assert sum(got["shares"]) == c["N"] and all(sum(t) == m for t, m in zip(got["trips"], got["shares"]))


def test_what_the_rows_are_there_for():
    """The properties of the launches that the table's last column names, beyond the single figures."""
    # B1, B2: the thread-per-glowworm kernel's main loop makes a second, partly filled trip -- the launch's own choice
    for case in ("B1", "B2"):
        c = CASES[case]
        assert c["S"] * c["N"] > gso_shapes.PHASED_UP_TO
        for k2 in c["k2"]:
            shape = launch(c["S"], c["N"], k2)
            assert shape["kernel"] == "single" and all(len(t) == 2 and t[0] == 1024 and 0 < t[1] < 64 for t in shape["trips"])
    assert launch(256, 2100, None)["lds"] > 64 * 1024
    # B3: three trips of the phased kernel, the last of 2 of 128 groups, on the second walk
    b3 = launch(128, 1030, "phased")
    assert b3["second_walk"] and b3["trips"][0] == [128, 128, 2]
    starts = np.cumsum([0] + b3["shares"][:-1])
    assert tuple(int(s) + k for s in starts[:3] for k in (256, 257)) == B3_THIRD_TRIP
    # C1 / C2: either side of the line; C3: the largest swarm
    assert 48 * 3413 <= gso_shapes.LDS_LIMIT < 48 * 3414
    assert all(launch(1, 3413, k)["kernel"] == ("single" if k == "single" else "phased") for k in K2_ALL)
    assert all(launch(1, 3414, k)["kernel"] == "single" for k in K2_ALL)
    assert CASES["C3"]["N"] == gso_shapes.MAX_GLOWWORMS
    # A2 / A3 / A5 in the phased kernel: groups without a glowworm take part in the second walk's votes
    for case in ("A2", "A3", "A5"):
        shape = launch(1, CASES[case]["N"], "phased")
        assert shape["second_walk"] and all(shape["threads"] // 8 > m for m in shape["shares"])
    # A1, A4: three words of kept verdicts
    assert launch(1, 130, None)["words"] == 3
    # the shares of test_gso_odd_sizes' 1030 glowworms in one swarm are far below a workgroup
    assert launch(1, 1030, "single")["share"] == 61 and launch(1, 1030, "single")["parts"] == 17


def _margins(before, after):
    """(smallest |l_i - l_j| over pairs inside vr_i + 1e-6 with non-identical poses, smallest |d - vr_i| over pairs with
    l_j > l_i, largest neighbour count recomputed here) of one step."""
    pos, vr, rows = before["poses"][:, :3], before["vision_range"], before["poses"]
    luc = after["luciferin"]
    n = len(luc)
    gap_l, gap_d = np.inf, np.inf
    counts = np.zeros(n, dtype=np.int64)
    for lo in range(0, n, 512):
        hi = min(n, lo + 512)
        dx, dy, dz = (pos[lo:hi, None, k] - pos[None, :, k] for k in range(3))
        d = np.sqrt(dx * dx + dy * dy + dz * dz)               # glowworm.rs:193-202, in its order
        dl = luc[None, :] - luc[lo:hi, None]
        other = np.arange(n)[None, :] != np.arange(lo, hi)[:, None]
        near = other & (d < vr[lo:hi, None] + 1e-6)
        for a, b in zip(*np.nonzero(near & (d == 0.0))):      # identical poses are left out of the luciferin margin
            if np.array_equal(rows[lo + a], rows[b]):
                near[a, b] = False
        if near.any():
            gap_l = min(gap_l, np.abs(dl[near]).min())
        brighter = other & (dl > 0.0)
        if brighter.any():
            gap_d = min(gap_d, np.abs(d - vr[lo:hi, None])[brighter].min())
        counts[lo:hi] = (brighter & (d < vr[lo:hi, None])).sum(axis=1)
    assert np.array_equal(counts, after["n_neighbors"])      # the numpy restatement reads the same state as the oracle
    return gap_l, gap_d


def _unit(q):
    return q / np.linalg.norm(q, axis=1, keepdims=True)


@pytest.mark.parametrize("case", sorted(CASES))
def test_margins_and_paths(shapes, case):
    c = CASES[case]
    n = c["N"]
    replays = shapes.replay(case)
    assert sorted(replays) == sorted(sampled_swarms(case))
    for swarm, states in replays.items():
        assert len(states) == c["steps"] + 1
        flips = linear = 0
        most, none = 0, False
        moved_ever = np.zeros(n, dtype=bool)
        for before, after in zip(states[:-1], states[1:]):
            gap_l, gap_d = _margins(before, after)
            print("%s swarm %d: luciferin gap %.3g, range gap %.3g, moved %d" % (case, swarm, gap_l, gap_d, after["moved"].sum()))
            assert gap_l >= MIN_LUCIFERIN_GAP, (case, swarm)
            assert gap_d >= MIN_RANGE_GAP, (case, swarm)
            moved = after["moved"] != 0
            assert np.array_equal(moved, after["target"] != np.arange(n))
            q = _unit(before["poses"][:, 3:7])
            dot = (q[moved] * q[after["target"][moved]]).sum(axis=1)
            flips += int((dot < 0.0).sum())
            linear += int((np.abs(dot) > LINEAR_THRESHOLD).sum())
            most = max(most, int(after["n_neighbors"].max()))
            none = none or bool((after["n_neighbors"] == 0).any())
            moved_ever |= moved
        last = states[-1]["moved"] != 0
        print("%s swarm %d: %d sign flips, %d linear slerps, %d moved at the last step, up to %d neighbours"
              % (case, swarm, flips, linear, last.sum(), most))
        if case.startswith("A"):
            assert flips >= 1 and linear >= 1      # both branches of the slerp (src/qt.rs:67-91), and the sign flip
            assert last.sum() >= n / 4
            assert most > 5 and none                # a vision range that shrinks, one that grows
        if case == "B1":
            assert last[1024:].any()               # the second trip's 6 threads
        if case == "B2":
            assert last[1024:1050].any() and last[2074:2100].any()
        if case == "B3":
            assert moved_ever[list(B3_THIRD_TRIP)].any()
        if case.startswith("C"):
            assert last.sum() >= n / 2
