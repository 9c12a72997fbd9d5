"""tests/bsas_edges.py on the CPU: the integer oracle is the tool's rule, and every case built for tests/test_gpu_bsas_edges.py
is what it says -- the intended S is realised, nothing is a tie, every threshold list decides in at floor(s*) and out one above."""
import math
import os

import numpy as np
import pytest

import bsas_edges as be
from test_analysis_cpu import CZY, Restated, analyse_module, czy_restated
from test_ranked_cpu import RankedRestated

GRID_CUTOFFS = (0.0, 0.0001, 0.5, 1.0, 2.0, 3.9999, 4.0, 10.0, 12.5, 30.0)
GRID_N = list(range(1, 1001)) + [1281, 4096, 6681]


# ---- the oracle against the tool's rule ---------------------------------------------------------------------------------------

def test_the_integer_rule_is_the_tools_rule_around_every_threshold():
    """within() against Python's round(math.sqrt(S * 1e-6 / n), 4) <= cutoff (lgd_cluster_bsas.py) and numpy's
    rint(sqrt(S * 1e-6 / n) * 1e4) / 1e4 <= cutoff (the kernels' expression), S within 2 of s*.  Ties are counted and they are the
    only cases left out."""
    cases = ties = 0
    for cutoff in GRID_CUTOFFS:
        for n in GRID_N:
            f = be.s_floor(n, cutoff)
            for S in range(max(0, f - 2), f + 3):
                cases += 1
                if be.is_tie(S, n, cutoff):
                    ties += 1
                    assert n % 16 == 0 and S == f
                    continue
                want = be.within(S, n, cutoff)
                assert (round(math.sqrt(S * 1e-6 / n), 4) <= cutoff) == want, (S, n, cutoff)
                assert bool(np.rint(np.sqrt(S * 1e-6 / n) * 1e4) / 1e4 <= cutoff) == want, (S, n, cutoff)
                assert want == (S <= f)
    print("%d cases, %d ties left out" % (cases, ties))
    assert (cases, ties) == (48820, 20)


def test_threshold_K_and_the_ends_of_the_cutoff_range():
    assert [be.threshold_K(c) for c in (0.0, 0.0001, 0.5, 4.0, 30.0)] == [0, 1, 5000, 40000, 300000]
    assert be.threshold_K(-1.0) is None and be.threshold_K(be.INF) == be.INF and be.threshold_K(-0.0) == 0
    assert be.threshold_K(0.00015) == 1 and be.threshold_K(3.99999) == 39999
    assert not be.within(0, 7, -1.0) and not be.within(0, 7, -1e-300) and be.within(10 ** 30, 7, be.INF)
    assert be.within(0, 7, 0.0) and not be.within(1, 7, 0.0) and be.within(1, 401, 0.0)
    assert be.s_floor(175, 4.0) == 2800070000 and be.s_floor(7, 4.0) == 112002800     # s* = 2 800 070 000.4375 at n = 175
    assert be.is_tie(400 * 9 // 400, 400, 0.0001) and not be.is_tie(9, 401, 0.0001)


def test_printed_thousandths_read_the_decimal_expansion():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.uniform(-300, 300, 2000), np.arange(-40, 40) / 16.0 + 0.0005, [0.0005, 1.0005, 2.5, -0.0005, 1e-9, -1e-9, -0.0]])
    assert [be.printed_thousandths(v) for v in x] == [int(("%.3f" % v).replace(".", "")) for v in x]
    assert be.printed_thousandths(be.LARGEST) == 2 ** 31 - 1 and be.printed_thousandths(be.REFUSED) == 2 ** 31
    assert be.printed_thousandths(0.0005) == 1                                            # the double lies above the half
    assert be.printed_thousandths(0.0625) == 62 and be.printed_thousandths(0.1875) == 188   # exact halves go to the even


def test_sums_of_squares():
    for S in list(range(0, 300)) + [be.s_floor(n, 4.0) + d for n in (7, 31, 175, 97, 98) for d in (0, 1)] + [4 * 10 ** 10, 87300290997]:
        six = be.squares(S)
        assert sum(v * v for v in six) == S
        assert (be.three_squares(S) is None) == any(six[3:])
        if S:
            one, three = be.split(S)
            assert one[0] ** 2 + sum(v * v for v in three) == S and any(three) and not any(one[1:])
        assert sum(v * v for v in be.four_squares(S)) == S
    assert sum(be.three_squares(be.s_floor(n, 4.0) + d) is None for n in (7, 31, 175) for d in (0, 1)) > 0   # why four are needed


def test_the_oracle_reproduces_the_golden_clusters_of_two_swarms():
    """cluster.repr of 1czy swarms 0 and 9, from the thousandths the Python tool re-reads (Restated.backbone_printed)."""
    an = analyse_module()
    rs = czy_restated()
    for s in (0, 9):
        poses, cols = an.read_gso(os.path.join(CZY, "swarm_%d" % s, "gso_100.out"))
        T = np.array([np.rint(rs.backbone_printed(p) * 1000.0).astype(np.int64).ravel() for p in poses])
        cluster_of, reps, ties = be.bsas(T, len(rs.backbone), cols["scoring"], 4.0)
        assert ties == 0
        lines = an.cluster_repr_lines(np.array(cluster_of), np.array(reps), len(reps), cols["scoring"])
        assert "".join(lines) == open(os.path.join(CZY, "swarm_%d" % s, "cluster.repr")).read()


# ---- every built case ---------------------------------------------------------------------------------------------------------

def test_no_case_is_a_tie_and_every_intended_sum_is_realised():
    cases = comparisons = 0
    for case in be.all_cases():
        cases += 1
        for measure, (cluster_of, reps, ties) in case.expected.items():
            assert ties == 0, (case.name, measure)
            assert len(cluster_of) == len(case.poses) and min(cluster_of) == 0 and max(cluster_of) == len(reps) - 1
            if case.swarms is not None and measure == "complex":
                assert all(t == 0 for _, _, t in be.swarm_expected(case)), case.name
        T = be.table(case.spec, case.poses, next(iter(case.expected)))
        for i, j, S in case.intended:
            comparisons += 1
            assert be.sum_sq(T[i], T[j]) == S, (case.name, i, j)
    print("%d cases, %d intended sums, none a tie" % (cases, comparisons))
    assert cases > 150 and comparisons > 900


def test_every_posed_coordinate_of_the_exact_cases_is_a_whole_thousandth():
    worst = 0.0
    for case in be.exact_cases():
        x = be.posed(case.spec, case.poses) * 1000.0
        worst = max(worst, float(np.max(np.abs(x - np.rint(x)))))
    print("farthest from a whole thousandth: %.3g" % worst)
    assert worst < 1e-6


@pytest.mark.parametrize("n,measure", be.THRESHOLD_GROUPS)
def test_threshold_lists_decide_in_at_the_floor_and_out_one_above(n, measure):
    for case in be.threshold_cases(n, measure):
        assert be.n_measured(case.spec, measure) == n
        cluster_of, reps, _ = case.expected[measure]
        sums = {S: i for i, _, S in case.intended}
        K = be.threshold_K(case.cutoff)
        if K is None:
            assert cluster_of == list(range(len(case.poses))) and 0 in sums     # a pose equal to the representative is out too
        elif K == be.INF:
            assert set(cluster_of) == {0} and len(sums) >= 3
        else:
            f = be.s_floor(n, case.cutoff)
            assert f in sums and f + 1 in sums, case.name
            assert cluster_of[sums[f]] == 0 and cluster_of[sums[f + 1]] != 0
            assert 400 * f < n * (2 * K + 1) ** 2 < 400 * (f + 1)
            pairs = be.swarm_expected(case, measure)
            assert pairs[sums[f] - 1][0] == [0, 0] and pairs[sums[f + 1] - 1][0] == [0, 1]


@pytest.mark.parametrize("layout,measure", be.WHERE_GROUPS)
def test_where_cases_put_the_deciding_term_in_every_mover_and_pair(layout, measure):
    spec = be.LAYOUTS[layout]
    n = be.n_measured(spec, measure)
    f = be.s_floor(n, be.WHERE_CUTOFF)
    movers = be.movers_of(spec, measure)
    for fillers in be.WHERE_FILLERS:
        case = be.where_case(layout, measure, fillers)
        cluster_of, reps, _ = case.expected[measure]
        assert len(case.intended) == 2 * len(movers) ** 2 and cluster_of[:1 + fillers] == list(range(1 + fillers))
        for i, _, S in case.intended:
            assert S in (f, f + 1) and (cluster_of[i] == 0) == (S == f)
            assert fillers == 0 or i >= 64          # behind the first candidate block
        # a split probe's partial sum over the first mover alone is within: the walk cannot stop early
        X = be.table(spec, case.poses, measure)
        for i, _, S in case.intended[2 * len(movers):]:
            moved = np.flatnonzero(X[i] != X[0]) // 3
            assert len(set(moved)) == 2
            for atom in set(moved):
                part = be.sum_sq(X[i][3 * atom:3 * atom + 3], X[0][3 * atom:3 * atom + 3])
                assert 0 < part < S and be.within(part, n, be.WHERE_CUTOFF)
    # the layouts reach the granule edges of both walks
    order_bsas = [p for p in spec.rec_movers] + [spec.n_rec_bb + p for p in spec.lig_movers]
    assert all(0 <= p < spec.n_rec_bb + spec.n_lig_bb for p in order_bsas)


def test_the_layouts_cover_the_granule_edges_of_both_walks():
    bsas_at, ranked_at, walks = set(), set(), set()
    for spec in be.LAYOUTS.values():
        n = spec.n_rec_bb + spec.n_lig_bb
        for p in [q for q in spec.rec_movers] + [spec.n_rec_bb + q for q in spec.lig_movers]:
            bsas_at.add("last" if p == n - 1 else p)
        walk = spec.n_lig_bb + (spec.n_rec_bb if spec.rec_movers else 0)
        walks.add(walk)
        for p in [q for q in spec.lig_movers] + [spec.n_lig_bb + q for q in spec.rec_movers]:
            ranked_at.add("last" if p == walk - 1 else p)
    assert {0, 31, 32, 63, 64, "last"} <= bsas_at and {0, 31, 32, 63, 64, "last"} <= ranked_at
    assert {20, 32, 33, 65, 97} <= walks and any(n % 32 == 1 for n in walks)


def ranked_position(case, i):
    return sorted(range(len(case.poses)), key=lambda j: (-case.scoring[j], j)).index(i)


@pytest.mark.parametrize("measure", be.MEASURES)
def test_ranked_position_cases_stand_where_they_say(measure):
    f = be.s_floor(be.n_measured(be.POSITION_SPEC, measure), be.POSITION_CUTOFF)
    for pos in be.POSITIONS:
        case = be.position_case(measure, pos)
        cluster_of, reps, _ = case.expected[measure]
        assert len(reps) == pos + 1                                  # the leader, the fillers, the probe that is out
        at = {S: i for i, _, S in case.intended}
        assert sorted(ranked_position(case, i) for i in at.values()) == [pos, pos + 1]
        assert ranked_position(case, at[f]) == (pos + 1 if pos in (255, 300) else pos)
        assert cluster_of[at[f]] == 0 and cluster_of[at[f + 1]] == pos
    for joins in (1, 2):
        for fillers in (0, 70):
            case = be.two_leader_case(measure, joins, fillers)
            cluster_of, reps, _ = case.expected[measure]
            (l2, _, W), (probe, _, s1), (_, _, s2) = case.intended
            assert W > f + 1 and s2 == f and s1 == f + (joins == 2)
            assert cluster_of[l2] == 1 and cluster_of[probe] == joins - 1 and len(reps) == 2 + fillers
            assert ranked_position(case, probe) == 2 + fillers


# ---- half-thousandths ---------------------------------------------------------------------------------------------------------

PLAIN_RINT_WRONG = 100      # of the 500 poses at a half; the count itself is printed


def test_half_thousandths_round_both_ways_and_a_plain_rint_gets_many_wrong():
    values = be.half_values()
    printed = [be.printed_thousandths(t) for _, t, _, _ in values]
    assert all(p in (k, k + 1) for p, (k, _, _, _) in zip(printed, values))
    assert all(be.printed_thousandths(lo) == k and be.printed_thousandths(hi) == k + 1 for k, _, lo, hi in values)
    up = sum(p == k + 1 for p, (k, _, _, _) in zip(printed, values))
    wrong = sum(int(np.rint(t * 1000.0)) != p for p, (_, t, _, _) in zip(printed, values))
    by_size = [sum(int(np.rint(t * 1000.0)) != p for p, (k, t, _, _) in zip(printed, values) if lo_ <= abs(k) < hi_)
               for lo_, hi_ in ((0, 1000), (1000, 10 ** 6), (10 ** 6, 10 ** 9))]
    print("%d poses at a half: %d print up, %d down; rint(x * 1000) is wrong for %d (by size: %r)" % (len(values), up, len(values) - up, wrong, by_size))
    assert up >= 100 and len(values) - up >= 100
    assert wrong >= PLAIN_RINT_WRONG and all(by_size)
    for which in be.HALF_SPECS:
        case = be.half_case(which)
        for cluster_of, reps, ties in case.expected.values():
            assert ties == 0
        for (cluster_of, reps, _), p, (k, _, _, _) in zip(be.swarm_expected(case), printed, values):
            assert cluster_of == ([0, 0, 1] if p == k else [0, 1, 0])


# ---- the old sweep ------------------------------------------------------------------------------------------------------------

def test_the_200_pose_sweeps_of_the_older_tests_never_come_near_the_threshold():
    """test_knife_edge_decisions_equal_the_restatement of tests/test_gpu_analysis.py and tests/test_gpu_ranked.py step the ligand
    across 3.99 - 4.01 A: the nearest S they produce is thousands of units from s*, which is why tests/bsas_edges.py exists."""
    rr = RankedRestated(Restated(os.path.join(CZY, "lightdock_1czy_protein.pdb"), os.path.join(CZY, "lightdock_1czy_peptide.pdb")))
    nb, n_lig = len(rr.atoms["complex"]), len(rr.atoms["ligand"])
    assert (nb, n_lig) == (175, 7)
    d = np.array([1.0, 0.37, -0.52]) / np.linalg.norm([1.0, 0.37, -0.52])
    for measure, n in (("complex", nb), ("ligand", n_lig)):
        scale = np.sqrt(nb / n_lig) if measure == "complex" else 1.0
        poses = np.zeros((200, 7))
        poses[:, 3] = 1.0
        poses[1:, :3] = (np.linspace(3.99, 4.01, 199) * scale)[:, None] * d
        trace = []
        _, reps, ties = be.bsas(rr.thousandths(poses, measure), n, 100.0 - np.arange(200.0), 4.0, trace)
        nearest = min(abs(400 * S - n * 80001 ** 2) for S in trace) / 400.0
        print("%s: %d comparisons, %d clusters, nearest |S - s*| = %.1f" % (measure, len(trace), len(reps), nearest))
        assert ties == 0 and len(reps) > 1 and nearest > 1000.0


# ---- ties ---------------------------------------------------------------------------------------------------------------------

def test_the_tie_cases_are_ties_where_the_float_path_holds_at_S_and_fails_one_double_above():
    """So the largest double for which the float path holds -- ranked_begin's s_max -- is the integer S itself."""
    cases = be.tie_cases()
    assert len(cases) == 2 * len(be.TIES)
    for spec, poses, scoring, cutoff, S in cases:
        n = spec.n_rec_bb + spec.n_lig_bb
        T = be.table(spec, poses, "complex")
        assert be.sum_sq(T[0], T[1]) == S and be.is_tie(S, n, cutoff) and not be.within(S, n, cutoff)
        assert be.float_path(S, n, cutoff) and not be.float_path(np.nextafter(np.float64(S), np.inf), n, cutoff)
        assert be.float_path(S - 1, n, cutoff) and not be.float_path(S + 1, n, cutoff)
