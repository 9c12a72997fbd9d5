"""The cross-link rule (ld_complex_crosslinks, lightdock-rust_amd/xlinks.py) on the CPU: the numpy restatement
of tests/xlink_reference.py (the checker the GPU tests use) held to an independent heapq Dijkstra on small boxes and to
values the rule's text pins, the exact square root at squares +- 1, the symmetry of D, and xlinks.py's link file parser,
judgement, ordering and text on made-up numbers."""
import heapq
import math

import numpy as np
import pytest

import xlink_reference as xr
from test_analysis_cpu import tool_module

C, N, O = 1700, 1550, 1520


def dijkstra(t, radii, a, b, p, h, rho, M):
    """D(a, b) from the rule's text alone: nodes as integer triples in a dict, a heap, no arrays."""
    part = [(tuple(int(v) for v in t[x]), int(radii[x]) + p) for x in range(len(t)) if radii[x] > 0]
    ca, cb = [int(v) for v in t[a]], [int(v) for v in t[b]]
    lo = [-((-(c - M)) // h) for c in ca]
    hi = [(c + M) // h for c in ca]
    free = {}

    def is_free(q):
        if q not in free:
            free[q] = all(l <= v <= u for v, l, u in zip(q, lo, hi)) and \
                all(sum((v * h - c) ** 2 for v, c in zip(q, x)) >= E * E for x, E in part)
        return free[q]

    def near(c):
        r = range(-(rho // h) - 1, rho // h + 2)
        base = [v // h for v in c]
        for i in r:
            for j in r:
                for k in r:
                    q = (base[0] + i, base[1] + j, base[2] + k)
                    d2 = sum((v * h - x) ** 2 for v, x in zip(q, c))
                    if d2 <= rho * rho and is_free(q):
                        yield q, math.isqrt(d2)

    w = (0, h, math.isqrt(2 * h * h), math.isqrt(3 * h * h))
    heap = [(s, q) for q, s in near(ca)]
    heapq.heapify(heap)
    done = {}
    while heap:
        d, q = heapq.heappop(heap)
        if q in done or d > M:
            continue
        done[q] = d
        for dx, dy, dz in xr.SHIFTS:
            r = (q[0] + dx, q[1] + dy, q[2] + dz)
            if r not in done and is_free(r):
                heapq.heappush(heap, (d + w[abs(dx) + abs(dy) + abs(dz)], r))
    best = min((done[q] + s for q, s in near(cb) if q in done), default=xr.NO_PATH)
    return best if best <= M else xr.NO_PATH


# ---- the exact square root --------------------------------------------------------------------------------------

def test_isqrt_at_squares_plus_and_minus_one():
    roots = np.array([1, 2, 3, 999, 1000, 1700, 2999, 3000, 6000, 46340, 46341, 60000, 103923, 10 ** 6, 2 ** 26 + 1], dtype=np.int64)
    assert np.array_equal(xr.isqrt(roots * roots), roots)
    assert np.array_equal(xr.isqrt(roots * roots - 1), roots - 1)
    assert np.array_equal(xr.isqrt(roots * roots + 1), roots)
    assert np.array_equal(xr.isqrt(roots * roots + 2 * roots), roots)
    assert xr.isqrt(np.array([0, 1, 2, 3, 4])).tolist() == [0, 1, 1, 1, 2]
    for h in (500, 707, 1000, 1999, 2000):
        w1, w2, w3 = xr.weights(h)
        assert w1 == h and w2 * w2 <= 2 * h * h < (w2 + 1) ** 2 and w3 * w3 <= 3 * h * h < (w3 + 1) ** 2
        assert h <= w2 <= w3 < 2 * h and 60000 + w3 < 0xFFFF                 # what the level sweep and the 16-bit field lean on
    assert xr.weights(1000) == (1000, 1414, 1732)


def test_parameters_and_their_bounds():
    assert xr.parameters() == (0, 1000, 3000, 35000)
    assert xr.parameters(2.0, 0.5, 6.0, 40.0) == (2000, 500, 6000, 40000) and xr.parameters(0.0, 2.0, 0.001, 2.0) == (0, 2000, 1, 2000)
    assert xr.parameters(0.0, 0.75, 3.0, 60.0)[3] // 750 == 80
    for bad in ((-0.001,), (2.001,), (0.0, 0.4994), (0.0, 2.0006), (0.0, 1.0, 0.0004), (0.0, 1.0, 6.0006), (0.0, 1.0, 3.0, 0.9994), (0.0, 1.0, 3.0, 60.0006),
                (0.0, 0.5, 3.0, 40.5), (float("nan"),), (0.0, float("inf")), (0.0, 1.0, -float("inf")), (0.0, 1.0, 3.0, 1e300)):
        with pytest.raises(xr.Refused):
            xr.parameters(*bad)


# ---- values the text pins ---------------------------------------------------------------------------------------

def test_two_carbons_a_lone_carbon_a_hydrogen_and_the_cap():
    t = np.array([[0, 0, 0], [0, 5000, 0], [10000, 0, 0]])       # C, H, C
    radii = np.array([C, 0, C])
    links = [(0, 2), (2, 0), (0, 0), (1, 1), (0, 1)]
    assert xr.straight2(t, links) == [10 ** 8, 10 ** 8, 0, 0, 25 * 10 ** 6]
    # along the axis: the doors (2, 0, 0) and (8, 0, 0), two hops of 2000 and six moves of 1000; about a lone carbon the
    # nearest free node is (1, 1, 1), a hop of isqrt(3 000 000) there and back; the hydrogen stands on a free node
    assert xr.path_lengths(t, radii, links, max_length=12.0).tolist() == [10000, 10000, 3464, 0, 5000]
    assert xr.path_lengths(t, radii, links[:1], max_length=10.0).tolist() == [10000]            # D == M is reported
    assert xr.path_lengths(t, radii, links[:1], max_length=9.999).tolist() == [xr.NO_PATH]      # D == M + 1 is not
    assert xr.path_lengths(t, radii, links[:4], reach=1.0, max_length=12.0).tolist() == [xr.NO_PATH, xr.NO_PATH, xr.NO_PATH, 0]   # no door
    # the strict rim: (2, 0, 0) is free at E = 2000 and blocked at E = 2001; with a reach of 2 A it was the last door
    assert xr.path_lengths(t, np.array([2000, 0, 2000]), links[:1], reach=2.0, max_length=12.0).tolist() == [10000]
    assert xr.path_lengths(t, np.array([2001, 0, 2001]), links[:1], reach=2.0, max_length=12.0).tolist() == [xr.NO_PATH]
    # a door at exactly rho: (3, 0, 0) is the only free node within 3000 of a blocker of E = 3000 -- none within 2999
    wide = np.array([3000, 0, 3000])
    assert xr.path_lengths(t, wide, links[:1], reach=3.0, max_length=12.0).tolist() == [10000]
    assert xr.path_lengths(t, wide, links[:1], reach=2.999, max_length=12.0).tolist() == [xr.NO_PATH]
    with pytest.raises(xr.Refused):
        xr.path_lengths(np.array([[0, 0, 0], [10 ** 9 + 1, 0, 0]]), np.array([C, C]), [(0, 0)])
    with pytest.raises(xr.Refused):
        xr.path_lengths(t, np.zeros(3, dtype=np.int64), links)


# ---- against Dijkstra -------------------------------------------------------------------------------------------

def clump(rng, n, spread):
    t = rng.integers(-spread, spread, (n, 3)).astype(np.int64)
    radii = rng.choice([0, C, N, O, 1800], n).astype(np.int64)
    radii[0] = C
    return t, radii


def test_restatement_against_heapq_dijkstra_on_small_boxes():
    rng = np.random.default_rng(11)
    seen = set()
    for case, (probe, cell, reach, max_length) in enumerate(((0.0, 1.0, 3.0, 9.0), (1.4, 1.0, 3.0, 9.0), (0.0, 0.5, 2.0, 4.5), (0.5, 2.0, 4.5, 18.0),
                                                             (2.0, 0.75, 6.0, 6.75))):
        p, h, rho, M = xr.parameters(probe, cell, reach, max_length)
        assert 2 * (M // h) + 1 <= 25
        for trial in range(2):
            t, radii = clump(rng, 10, 4500)
            t += np.array([0, 0, 0]) if trial == 0 else rng.integers(-10 ** 6, 10 ** 6, 3) * np.array([1, -1, 1])
            links = [(int(a), int(b)) for a, b in rng.integers(0, len(t), (3, 2))] + [(3, 3)]
            got = xr.path_lengths(t, radii, links, probe, cell, reach, max_length)
            want = [dijkstra(t, radii, a, b, p, h, rho, M) for a, b in links]
            assert got.tolist() == want, (case, trial)
            seen |= {"none" if v == xr.NO_PATH else "path" for v in want}
    assert seen == {"none", "path"}


def sheet_case(holes=0):
    """Two anchors that block nothing 6 A either side of a 9 x 9 sheet of carbons 1.5 A apart in the plane x = 0; `holes`:
    the middle (2 holes - 1)^2 atoms of the sheet are left out."""
    keep = [(i, j) for i in range(9) for j in range(9) if holes == 0 or max(abs(i - 4), abs(j - 4)) >= holes]
    t = np.array([(-6000, 0, 0), (6000, 0, 0)] + [(0, 1500 * (i - 4), 1500 * (j - 4)) for i, j in keep])
    return t, np.array([0, 0] + [C] * len(keep))


def test_a_wall_is_walked_round_and_a_hole_walked_through():
    link = [(0, 1)]
    t, radii = sheet_case()
    round_the_edge = xr.path_lengths(t, radii, link, max_length=25.0)[0]
    assert round_the_edge != xr.NO_PATH and round_the_edge > 12000 + 2 * 1000
    assert xr.path_lengths(t, radii, link, cell=2.0, max_length=24.0)[0] == dijkstra(t, radii, 0, 1, 0, 2000, 3000, 24000) != xr.NO_PATH
    # one atom left out: its place is 1500 from four carbons of radius 1700, so no node of the plane is free and nothing changes
    assert xr.path_lengths(*sheet_case(1), link, max_length=25.0)[0] == round_the_edge
    # the middle 5 x 5 left out: the origin is 4500 from the nearest carbon, free at probe 0 and at probe 1.4 (E = 3100)
    for probe in (0.0, 1.4):
        assert xr.path_lengths(*sheet_case(3), link, probe=probe, max_length=25.0)[0] == 12000


# ---- symmetry ---------------------------------------------------------------------------------------------------

def test_d_is_symmetric_whatever_the_source():
    rng = np.random.default_rng(5)
    for cell, max_length in ((1.0, 14.0), (0.7, 9.0), (2.0, 20.0)):
        t, radii = clump(rng, 20, 5000)
        t += np.array([-123457, 98765, 4321])
        pairs = [(int(a), int(b)) for a, b in rng.integers(0, len(t), (8, 2))]
        forward = xr.path_lengths(t, radii, pairs, 0.0, cell, 3.0, max_length)
        backward = xr.path_lengths(t, radii, [(b, a) for a, b in pairs], 0.0, cell, 3.0, max_length)
        assert forward.tolist() == backward.tolist() and (forward != xr.NO_PATH).any()


# ---- xlinks.py --------------------------------------------------------------------------------------------------

REC = [("A.LYS.45", "N"), ("A.LYS.45", "CA"), ("A.LYS.45", "NZ"), ("A.GLU.46", "CA"), ("A.GLU.46", "CA"), ("B.LYS.45", "CA")]
LIG = [("C.LYS.12", "N"), ("C.LYS.12", "CA"), ("C.LYS.12", "NZ"), ("C.ASP.13A", "CA")]


def test_link_file_parser():
    tool = tool_module("xlinks")
    text = ("# receptor, ligand, limit\n"
            "R A.LYS.45 NZ L C.LYS.12 NZ 30\n"
            "\n"
            "   L C.ASP.13A CA R B.LYS.45 CA 26.5   # a comment\n"
            "R A.LYS.45 CA R A.LYS.45 CA 0\n")
    links, limits, labels = tool.parse_links(text, REC, LIG)
    assert links == [(2, 6 + 2), (6 + 3, 5), (1, 1)] and limits == [30.0, 26.5, 0.0]
    assert labels == ["R:A.LYS.45:NZ-L:C.LYS.12:NZ", "L:C.ASP.13A:CA-R:B.LYS.45:CA", "R:A.LYS.45:CA-R:A.LYS.45:CA"]
    for bad, line, word in (("R A.LYS.45 NZ L C.LYS.99 NZ 30\n", 1, "no residue C.LYS.99"), ("\n\nR A.LYS.45 CB L C.LYS.12 NZ 30\n", 3, "no atom CB"),
                            ("R A.LYS.45 NZ L C.LYS.12 NZ 30\nR A.GLU.46 CA L C.LYS.12 NZ 30\n", 2, "more than one"),
                            ("R A.LYS.45 NZ L C.LYS.12 NZ\n", 1, "expected"), ("X A.LYS.45 NZ L C.LYS.12 NZ 30\n", 1, "expected"),
                            ("R A.LYS.45 NZ L C.LYS.12 NZ far\n", 1, "limit"), ("R A.LYS.45 NZ L C.LYS.12 NZ -1\n", 1, "limit"),
                            ("# one\nL A.LYS.45 NZ L C.LYS.12 NZ 30\n", 2, "no residue A.LYS.45 in the ligand")):
        with pytest.raises(ValueError) as e:
            tool.parse_links(bad, REC, LIG)
        assert str(e.value).startswith("line %d:" % line) and word in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        tool.parse_links("# nothing\n", REC, LIG)
    assert tool.atom_table(["A.LYS.45", "A.GLU.46"], [0, 0, 1], ["N", "CA", "CA"]) == [("A.LYS.45", "N"), ("A.LYS.45", "CA"), ("A.GLU.46", "CA")]
    with pytest.raises(ValueError):
        tool.atom_table(["A.LYS.45"], [0, 0], ["N"])


def test_judgement_ranking_and_text():
    tool = tool_module("xlinks")
    limits = [30.0, 10.0]
    straight2 = np.array([[400000000, 81000000], [400000000, 100000000], [900000000, 100000000], [961000000, 81000000]], dtype=np.uint64)
    path = np.array([[25000, 12500], [xr.NO_PATH, 10000], [30000, 10000], [31000, xr.NO_PATH]], dtype=np.uint32)
    straight, walked = tool.distances(straight2, path)
    assert straight.tolist() == [[20.0, 9.0], [20.0, 10.0], [30.0, 10.0], [31.0, 9.0]] and walked[0].tolist() == [25.0, 12.5] and np.isinf(walked[1, 0])
    satisfied, by_straight, violation = tool.judge(straight, walked, limits, 35.0)
    assert satisfied.tolist() == [1, 1, 2, 0] and by_straight.tolist() == [2, 2, 2, 1]
    assert violation.tolist() == [2.5, 5.0, 0.0, 1.0 + 25.0]        # without a path: max_length - limit
    assert tool.judge(straight, walked, [40.0, 10.0], 35.0)[2].tolist() == [2.5, 0.0, 0.0, 25.0]       # ... floored at 0
    order = tool.rank_rows(satisfied, violation)
    assert order == [2, 0, 1, 3]                                     # satisfied descending, then violation ascending
    assert tool.rank_rows([1, 1, 1], [0.5, 0.5, 0.25]) == [2, 0, 1]  # ... then the scoring rank
    only, same, v = tool.judge(straight, None, limits, 35.0)
    assert only.tolist() == same.tolist() == [2, 2, 2, 1] and v.tolist() == [0.0, 0.0, 0.0, 1.0]
    entries = [(2, 74, None, {"scoring": 31.28816735}), (0, 5, None, {"scoring": 20.5}), (7, 1, None, {"scoring": -2.5}), (3, 3, None, {"scoring": -3.0})]
    text = tool.rank_text(entries, order, satisfied, by_straight, violation, 2)
    assert text == (tool.HEADER +
                    "    7         1    -2.50000      2/2         2/2         0.000\n"
                    "    2        74    31.28817      1/2         2/2         2.500\n"
                    "    0         5    20.50000      1/2         2/2         5.000\n"
                    "    3         3    -3.00000      0/2         1/2        26.000\n")
    assert tool.rank_text([], [], [], [], [], 2) == tool.HEADER
    listed = tool.links_text(order[:2], ["a-b", "c-d"], limits, straight, walked).splitlines()
    assert listed[0] + "\n" == tool.LINKS_HEADER and len(listed) == 5
    assert listed[1].split() == ["1", "a-b", "30.000", "30.000", "30.000"] and listed[4].split() == ["2", "c-d", "9.000", "12.500", "10.000"]
    assert tool.links_text([1], ["a-b", "c-d"], limits, straight, walked).splitlines()[1].split()[3] == "-"
    assert tool.links_text([1], ["a-b", "c-d"], limits, straight, None).splitlines()[2].split()[3] == "-"
