"""The premises of tests/gso_edges.py on the oracle alone (no GPU): every motif is ON the knife edge it is named after, at the
step it is built for, read from the oracle's own state before that step's moves; and a restatement of the movement phase in
plain Python floats (gso_edges.restate_step: is_neighbor, the vision update, the probabilities, the roulette with the draw
`step * N + i` of a ChaCha block of its own, move_towards with qslerp's normalisations and dot) gives the oracle's
n_neighbors, target, moved, vision range, translations and extents bit for bit at every step of every case, NaNs in the same
places -- the first time the roulette is checked against an exposed draw.  What tests/test_gpu_gso_edges.py then compares bit
for bit rests on this file: a case that does not reach its edge FAILS here.

Printed per edge: the case, the step and the glowworms that sit on it; per case min |sum - rnd| over all roulette stops.
"""
import math

import numpy as np
import pytest

import gso_edges
from gso_edges import CASES, KEPT, SECOND_WALK, STEPS, above, below, launch, motifs_of, sampled_swarms, same_bits

P_CASES = [c for c in CASES if CASES[c]["modes"] is None]
ANM_CASES = [c for c in CASES if CASES[c]["modes"] is not None]


@pytest.fixture(scope="module")
def edges(pkg, orc, tmp_path_factory):
    return gso_edges.edges(pkg, orc, str(tmp_path_factory.mktemp("gso_edges")))


def _distance(a, b):
    """src/glowworm.rs:193-202 in Python floats."""
    x1, y1, z1 = (float(c) for c in a[:3])
    x2, y2, z2 = (float(c) for c in b[:3])
    return math.sqrt((x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2) + (z1 - z2) * (z1 - z2))


class View:
    """The oracle's state before the moves of a step: poses and vision ranges after the previous step, luciferins after this one's
    update; and what the restatement saw at that step."""

    def __init__(self, edges, case, swarm=0):
        self.case, self.states, self.restated = case, edges.replay(case)[swarm], edges.restate(case, swarm)
        self.where = edges.swarm(case)[1]

    def poses(self, step):
        return self.states[step - 1]["poses"]

    def vision(self, step, i):
        return float(self.states[step - 1]["vision_range"][i])

    def luciferin(self, step, i):
        return float(self.states[step]["luciferin"][i])

    def d(self, step, i, j):
        return _distance(self.poses(step)[i], self.poses(step)[j])

    def event(self, step, i):
        return self.restated[step - 1][5][i]

    def after(self, step):
        return self.states[step]

    def pair(self, name):
        """(mover, other) of a two-member motif."""
        a, b = self.where[name]
        mover = self.where[name + ":mover"]
        return mover, (b if mover == a else a)


def _holding(kind):
    return [c for c in CASES if any(m[0] == kind for m in motifs_of(c))]


def _both_families(cases, edge):
    assert any(c in KEPT for c in cases) and any(c in SECOND_WALK for c in cases), \
        "%s needs a case that keeps its verdict bits and one on the second walk: %s" % (edge, cases)


# ---- the table of cases ------------------------------------------------------------------------------------------------------------

def test_case_table():
    assert sorted(CASES) == ["A11", "A32", "A32k", "M67", "N2", "N256", "N257", "N263", "N65", "N66", "N67", "N9"]
    assert {CASES[c]["N"] for c in P_CASES} == {2, 9, 65, 66, 67, 256, 257, 263}
    assert CASES["M67"]["S"] == 600 and all(CASES[c]["S"] == 1 for c in CASES if c != "M67")
    assert sorted(CASES[c]["modes"] for c in ANM_CASES) == [(1, 1), (3, 2), (3, 2)]
    assert {CASES[c]["N"] % 4 for c in ("N65", "N66", "N67")} == {1, 2, 3} and all(CASES[c]["N"] % 8 for c in ("N65", "N66", "N67", "N263"))
    for edge in ("E1", "E2at", "E2in", "E2out", "E3at", "E3in", "E4at", "E4in", "E4far", "E5x5", "E5x6", "E5x7", "E5x8", "E6", "E7x2",
                 "E7x3", "E7x6", "E10half", "E10recsame", "E10ligsame", "E10tiny", "E10huge"):
        _both_families(_holding(edge), edge)


@pytest.mark.parametrize("case", sorted(CASES))
def test_launch_arithmetic_of_the_table(case):
    """Every figure a row spells out is what the restated launch formulas of gso_shapes.launch give, in all three K2 settings."""
    c = CASES[case]
    assert set(c["expect"]) == set(gso_edges.K2_ALL)
    for k2 in gso_edges.K2_ALL:
        got = launch(c["S"], c["N"], k2)
        for key, want in c["expect"][k2].items():
            assert got[key] == want, (case, k2, key, got[key], want)
        assert got["second_walk"] == (c["N"] > 256) and (got["words"] > 0) == (c["N"] <= 256)


def test_the_values_on_the_edges():
    """Computed, not typed in: the quiet vision ranges, the offsets around kFarD2, the quaternions of the slerp's edges."""
    assert gso_edges.quiet_vision(0) == 0.2 and gso_edges.quiet_vision(1) == 0.2 + 0.08 * 5.0
    k5 = gso_edges.first_quiet_phase_at_5()
    assert gso_edges.quiet_vision(k5 - 1) < 5.0 and STEPS >= k5 + 3
    far = gso_edges.around_far_d2()
    print("EDGES kFarD2: D*D below / above at D =", repr(far["farlo"]), repr(far["farhi"]), "; D*D == 25.5:", repr(far.get("farat")))
    assert above(far["farlo"]) in (far.get("farat"), far["farhi"])
    rot = gso_edges.rotations()
    assert gso_edges.q_dot(*rot["eq"][:2]) == 0.9995 and gso_edges.q_dot(*rot["next"][:2]) == above(0.9995)
    assert math.copysign(1.0, gso_edges.q_dot(*rot["negzero"][:2])) == -1.0 and gso_edges.q_dot(*rot["negzero"][:2]) == 0.0
    assert math.copysign(1.0, gso_edges.q_dot(*rot["zero"][:2])) == 1.0
    assert abs(math.sqrt(sum(c * c for c in rot["norm2"][1])) - 2.0) < 1e-15


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_energy_is_the_staircase(edges, case):
    """The oracle's energy of every starting pose is 4.7 - 0.0157 v[bin(|t|)] bit for bit, the motifs' members are MARGIN from
    every bin edge and SEPARATION from every other motif, the fillers all score 4.7."""
    c = CASES[case]
    rows, where = edges.swarm(case)
    got = edges.cpu(c["modes"]).energy_rows(rows)
    members = {i: name for name, idx in where.items() if not name.endswith(":mover") for i in idx}
    for i, row in enumerate(rows):
        t = row[:3].copy()
        if c["modes"]:
            t[0] -= gso_edges.MODE_X * row[7]      # the receptor atom has moved along x: far below MARGIN unless the extent is huge
        b, edge = gso_edges.bin_of(t)
        assert got[i] == gso_edges.energy_of_bin(b), (case, i)
        if i in members:
            assert b is not None and edge >= gso_edges.MARGIN / 2, (case, i, edge)
        else:
            assert b is None and got[i] == 4.7 and math.sqrt(float(row[:3] @ row[:3])) > 40.0
    ids = sorted(members)
    for a in ids:
        for b in ids:
            if members[a] != members[b]:
                assert _distance(rows[a], rows[b]) > 5.6, (case, members[a], members[b])


# ---- the restatement against the oracle -------------------------------------------------------------------------------------------------

MARGINS = {}


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_is_the_oracle_bit_for_bit(edges, case):
    """n_neighbors, target, moved, vision range, translations, extents and the linear branch's rotations equal, NaNs in place;
    no roulette stop rests on a tie: min |sum - rnd| > 0, printed."""
    for swarm in sampled_swarms(case):
        restated = edges.restate(case, swarm)            # (a Panic of the reference would raise here)
        assert edges.agrees(case, swarm, restated) is None
        stops = [ev["margin"] for step in restated for ev in step[5].values() if "margin" in ev]
        assert stops, (case, swarm)
        MARGINS[(case, swarm)] = min(stops)
        print("EDGES %s swarm %d: %d roulette stops, min |sum - rnd| = %.3e" % (case, swarm, len(stops), min(stops)))
        assert min(stops) > 0.0


MUTATIONS = [("d<=vr", ["N9", "N263"]), ("li<=lj", ["N9", "N263"]), ("far", ["N66", "N263"]), ("dot>=", ["N2", "N257"]),
             ("&31", ["N256"]), ("nofmax", ["N65", "N257"])]


@pytest.mark.parametrize("mutation,cases", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_a_mutated_restatement_disagrees_with_the_oracle(edges, mutation, cases):
    """The kernel mutations of the issue, applied to the restatement: `d <= vr`, `li <= lj`, kFarD2 = 24.9, `dot >= 0.9995`,
    the kept bits' `& 63` as `& 31`, `fmax(0, v)` dropped.  Each must show against the oracle in a case that keeps its verdict bits
    and in one on the second walk (`& 31`: kept bits only).  (The scan tail's `j < j_end` cannot be restated: without it the
    thread-per-glowworm kernel reads LDS beyond the swarm, whose content nothing defines; the phased kernel's is_neighbour refuses
    j >= N on its own.)"""
    for case in cases:
        try:
            what = edges.agrees(case, 0, edges.restate(case, 0, mutate=(mutation,)))
        except gso_edges.Panic as panic:
            what = "the reference would panic: %s" % panic
        print("EDGES mutation %-7s in %-5s shows as: %s" % (mutation, case, what))
        assert what is not None, (mutation, case)


# ---- the motifs are on their edges ------------------------------------------------------------------------------------------------------

def _views(edges, kind):
    cases = _holding(kind)
    assert cases, kind
    return [View(edges, c) for c in cases]


def test_e1_luciferin_tie_inside_the_vision_range(edges):
    for v in _views(edges, "E1"):
        a, b = v.where["E1"]
        for step in range(1, STEPS + 1):
            assert v.luciferin(step, a) == v.luciferin(step, b)
            assert v.d(step, a, b) < min(v.vision(step, a), v.vision(step, b))
            assert v.event(step, a)["cnt"] == 0 and v.event(step, b)["cnt"] == 0
            assert v.after(step)["n_neighbors"][a] == 0 and v.after(step)["n_neighbors"][b] == 0
        print("EDGES E1 %s: glowworms %d, %d tie at l = %r, d = %r, every step" % (v.case, a, b, v.luciferin(1, a), v.d(1, a, b)))
    _both_families(_holding("E1"), "E1")


def test_e2_distance_equals_the_vision_range_at_step_1(edges):
    for name, offset, is_neighbour in (("E2at", 0.2, False), ("E2in", below(0.2), True), ("E2out", above(0.2), False)):
        for v in _views(edges, name):
            i, j = v.pair(name)
            assert v.vision(1, i) == 0.2 and v.luciferin(1, i) < v.luciferin(1, j)
            assert v.d(1, i, j) == offset
            assert v.after(1)["n_neighbors"][i] == (1 if is_neighbour else 0) and v.after(1)["moved"][i] == (1 if is_neighbour else 0)
            if not is_neighbour:     # ... and at step 2 it is one: the pair was held apart by the edge alone
                assert v.after(2)["n_neighbors"][i] == 1 and v.after(2)["target"][i] == j
            print("EDGES %s %s: step 1, glowworm %d seeks %d at d = %r, vr = 0.2: %s" % (name, v.case, i, j, v.d(1, i, j), "neighbour" if is_neighbour else "not a neighbour"))
        _both_families(_holding(name), name)


def test_e3_distance_equals_a_later_vision_range(edges):
    v2 = gso_edges.quiet_vision(2)
    for name, offset, first in (("E3at", v2, 4), ("E3in", below(v2), 3)):
        for v in _views(edges, name):
            i, j = v.pair(name)
            assert v.vision(3, i) == v2 and v.d(3, i, j) == offset and v.luciferin(3, i) < v.luciferin(3, j)
            for step in range(1, first):
                assert v.after(step)["n_neighbors"][i] == 0
            assert v.after(first)["n_neighbors"][i] == 1 and v.after(first)["target"][i] == j
            print("EDGES %s %s: step 3, glowworm %d seeks %d at d = %r, vr = %r: first a neighbour at step %d" % (name, v.case, i, j, offset, v2, first))
        _both_families(_holding(name), name)


def test_e4_vision_clamp_at_5_and_the_far_short_cut(edges):
    k5 = gso_edges.first_quiet_phase_at_5()
    far = gso_edges.around_far_d2()
    for v in _views(edges, "E4at"):
        i, j = v.pair("E4at")
        for step in range(1, STEPS + 1):
            assert v.after(step)["n_neighbors"][i] == 0 and v.d(step, i, j) == 5.0
        assert v.vision(k5, i) < 5.0 and all(v.vision(s, i) == 5.0 for s in range(k5 + 1, STEPS + 1)) and STEPS >= k5 + 3
        i, j = v.pair("E4in")
        assert v.d(k5 + 1, i, j) == below(5.0) and v.vision(k5 + 1, i) == 5.0 and v.luciferin(k5 + 1, i) < v.luciferin(k5 + 1, j)
        assert all(v.after(step)["n_neighbors"][i] == 0 for step in range(1, k5 + 1))
        assert v.after(k5 + 1)["n_neighbors"][i] == 1 and v.after(k5 + 1)["target"][i] == j
        print("EDGES E4 %s: vr reaches 5.0 at step %d; D = 5.0 never a neighbour, D = %r at step %d" % (v.case, k5 + 1, below(5.0), k5 + 1))
        for name, offset in [("E4far", 5.04)] + [("E4" + k, far[k]) for k in sorted(far)]:
            i, j = v.pair(name)
            d = v.d(1, i, j)
            assert d == offset and all(v.after(step)["n_neighbors"][i] == 0 for step in range(1, STEPS + 1))
            assert v.luciferin(STEPS, i) < v.luciferin(STEPS, j)
            print("EDGES %s %s: D = %r, D * D %s 25.5, never a neighbour" % (name, v.case, offset, "<" if d * d < 25.5 else "==" if d * d == 25.5 else ">"))
        assert far["farlo"] ** 2 < 25.5 < far["farhi"] ** 2
    _both_families(_holding("E4at"), "E4")


def test_e5_vision_clamp_at_0(edges):
    for c in (5, 6, 7, 8):
        name = "E5x%d" % c
        for v in _views(edges, name):
            idx = v.where[name]
            s = idx[0]
            assert v.event(1, s)["cnt"] == c and v.after(1)["n_neighbors"][s] == c and sorted(v.event(1, s)["neighbors"]) == sorted(idx[1:1 + c])
            want = min(5.0, max(0.0, 0.2 + 0.08 * float(5 - c)))
            assert float(v.after(1)["vision_range"][s]) == want and (c != 5 or want == 0.2) and (c != 8 or want == 0.0)
            assert 0.2 + 0.08 * float(5 - 8) < 0.0 < 0.2 + 0.08 * float(5 - 7)
            if c == 8:   # it has landed exactly on a brighter glowworm: d = 0 < 0 is false
                land = idx[-1]
                assert same_bits(v.poses(2)[s][:3], v.poses(2)[land][:3]) and v.d(2, s, land) == 0.0
                assert v.vision(2, s) == 0.0 and v.luciferin(2, s) < v.luciferin(2, land)
                assert v.after(2)["n_neighbors"][s] == 0 and v.after(2)["moved"][s] == 0
            print("EDGES %s %s: step 1, glowworm %d has %d neighbours, vision range %r afterwards" % (name, v.case, s, c, want))
        _both_families(_holding(name), name)


def test_e6_coincidence_and_nan(edges):
    for v in _views(edges, "E6"):
        a, b = v.pair("E6")
        assert v.after(1)["n_neighbors"][a] == 0 and v.vision(2, a) == 0.2 + 0.08 * 5.0 and v.luciferin(2, a) < v.luciferin(2, b)
        assert v.event(2, a)["norm"] == 0.5 and v.event(2, a)["coef"] == 1.0 and v.after(2)["target"][a] == b
        assert same_bits(v.after(2)["poses"][a][:3], v.after(2)["poses"][b][:3])
        assert v.d(3, a, b) == 0.0 and v.luciferin(3, a) < v.luciferin(3, b)
        assert v.event(3, a)["norm"] == 0.0 and v.event(3, a)["coef"] == math.inf and v.after(3)["target"][a] == b
        assert np.isnan(v.after(3)["poses"][a][:3]).all()
        for step in range(4, STEPS + 1):
            st = v.after(step)
            assert np.isnan(st["poses"][a][:3]).all() and st["scoring"][a] == 4.7 and np.isfinite(st["luciferin"][a])
            assert st["n_neighbors"][a] == 0 and st["moved"][a] == 0 and not (st["target"][np.arange(len(st["target"])) != a] == a).any()
        print("EDGES E6 %s: glowworm %d lands on %d at step 2 (coef == 1.0), norm == 0 at step 3: NaN from then on, scoring 4.7" % (v.case, a, b))
    _both_families(_holding("E6"), "E6")


def _fan_stops(v):
    """(step, seeker, event) of every roulette stop of a fan's seeker with at least two neighbours."""
    out = []
    for name in v.where:
        if name.startswith("E7") and not name.endswith(":mover"):
            s = v.where[name][0]
            out += [(step, s, v.event(step, s)) for step in range(1, STEPS + 1) if v.event(step, s)["cnt"] >= 2]
    return out


def test_e7_roulette_order_and_word_boundaries(edges):
    for family, label in ((KEPT, "kept bits"), (SECOND_WALK, "second walk")):
        seen = set()
        for case in family:
            if not any(m[0].startswith("E7") for m in motifs_of(case)):
                continue
            for swarm in sampled_swarms(case):
                v = View(edges, case, swarm)
                for name in sorted(v.where):
                    if not name.startswith("E7") or name.endswith(":mover"):
                        continue
                    idx = v.where[name]
                    s, nbrs = idx[0], sorted(idx[1:])
                    ev = v.event(6, s)          # first inside the vision range at step 6 (v5 = 2.2 > 1.87 > v4 = 1.8)
                    assert all(v.after(step)["n_neighbors"][s] == 0 for step in range(1, 6)), (case, name)
                    assert ev["neighbors"] == nbrs and len(set(ev["luciferins"])) == len(nbrs), (case, name)
                for step, s, ev in _fan_stops(v):
                    nb, place = ev["neighbors"], ev["place"]
                    seen.add("first" if place == 0 else "last" if place == len(nb) - 1 else "middle")
                    if nb[place] // 64 > nb[0] // 64:
                        seen.add("later word")
                    if len(set(ev["luciferins"])) == len(nb):
                        seen.add("unequal x%d" % len(nb))
                    print("EDGES E7 %s swarm %d: step %d, seeker %d, neighbours %s, place %d of %d, word %d (first neighbour's: %d)"
                          % (case, swarm, step, s, nb, place, len(nb), nb[place] // 64, nb[0] // 64))
        assert {"first", "middle", "last", "later word", "unequal x2", "unequal x3", "unequal x6"} <= seen, (label, seen)
    w256, w263 = edges.swarm("N256")[1], edges.swarm("N263")[1]
    assert w256["E7x2"][1:] == (63, 64) and w256["E7x3"][1:] == (127, 128, 130) and {191, 192, 255} <= set(w256["E7x6"][1:])
    assert edges.swarm("N67")[1]["E7x3"][0] == 63 and edges.swarm("N257")[1]["E7x3"][0] == 63 and w263["E7x3"][0] == 255


def test_e8_scan_tails(edges):
    """Neighbours at N-1, N-2, N-3 for N mod 4 = 1, 2, 3 (and N mod 8 != 0), found at step 6; a seeker at N-1."""
    for case in ("N65", "N66", "N67", "N263"):
        n = CASES[case]["N"]
        v = View(edges, case)
        idx = v.where["E7x3"]
        assert sorted(idx[1:]) == [n - 3, n - 2, n - 1] and n % 8 != 0
        assert v.event(6, idx[0])["neighbors"] == [n - 3, n - 2, n - 1]
        print("EDGES E8 %s: N mod 4 = %d, N mod 8 = %d, seeker %d finds %s at step 6" % (case, n % 4, n % 8, idx[0], [n - 3, n - 2, n - 1]))
    for case, name in (("N2", "E2in"), ("N257", "E7x2")):
        v = View(edges, case)
        s = v.where[name + ":mover"]
        assert s == CASES[case]["N"] - 1 and any(v.after(step)["moved"][s] for step in range(1, STEPS + 1))
        print("EDGES E8 %s: the seeker %d is glowworm N-1" % (case, s))


def test_e9_slerp_branches(edges):
    rot = gso_edges.rotations()
    seen = {}
    for case in P_CASES:
        v = View(edges, case)
        for name, kind, arg, idx, rot_name, anm_name in motifs_of(case):
            if rot_name is None:
                continue
            s = v.where[name + ":mover"]
            step = next(k for k in range(1, STEPS + 1) if v.after(k)["moved"][s])
            ev = v.event(step, s)
            mine, other, dot, branch, flip = rot[rot_name]
            assert same_bits(v.poses(step)[s][3:7], mine) and same_bits(v.poses(step)[ev_target(v, step, s)][3:7], other)
            want = gso_edges.q_dot(mine, other) if dot is None else dot
            assert same_bits([ev["dot"]], [want]) and ev["branch"] == branch and ev["flip"] == flip, (case, name, ev["dot"])
            seen.setdefault(rot_name, []).append(case)
            print("EDGES E9 %-7s %s: step %d, glowworm %d, dot = %r, %s branch%s" % (rot_name, case, step, s, ev["dot"], branch, ", flipped" if flip else ""))
    assert sorted(seen) == sorted(rot)
    for rot_name, cases in seen.items():
        _both_families(cases, "E9 " + rot_name)


def ev_target(v, step, s):
    return int(v.after(step)["target"][s])


def test_e10_anm_steps(edges):
    for case in ANM_CASES:
        k_rec, k_lig = CASES[case]["modes"]
        v = View(edges, case)
        for name, kind, arg, idx, rot_name, anm_name in motifs_of(case):
            s = v.where[name + ":mover"]
            assert v.after(1)["moved"][s] == 1
            ev, before, after = v.event(1, s), v.poses(1)[s], v.after(1)["poses"][s]
            rec_kind, lig_kind, cum_rec, cum_lig = gso_edges.ANM_SETTINGS[anm_name]
            assert same_bits([ev["cum_rec"], ev["cum_lig"]], [cum_rec, cum_lig]), (case, name, ev["cum_rec"], ev["cum_lig"])
            for kind_, lo, k in ((rec_kind, 7, k_rec), (lig_kind, 7 + k_rec, k_lig)):
                got = after[lo:lo + k]
                if kind_ == "unit":
                    assert got[0] == before[lo] + 0.5 and same_bits(got[1:], before[lo + 1:lo + k])
                elif kind_ == "unitneg":
                    assert got[0] == before[lo] - 0.5 and same_bits(got[1:], before[lo + 1:lo + k])
                elif kind_ == "same":
                    assert np.isnan(got).all()
                elif kind_ == "tiny":
                    assert got[0] == math.inf and np.isnan(got[1:]).all()
                else:
                    assert same_bits(got, before[lo:lo + k])
            print("EDGES E10 %-8s %s: step 1, glowworm %d, cum = %r (receptor), %r (ligand)" % (anm_name, case, s, ev["cum_rec"], ev["cum_lig"]))
    assert any(CASES[c]["modes"] == (1, 1) for c in ANM_CASES)
    _both_families([c for c in ANM_CASES if CASES[c]["modes"] == (3, 2)], "E10")
