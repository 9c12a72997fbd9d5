"""The collision cross-section rule (ld_complex_ccs, lightdock-rust_amd/ccs.py) on the CPU: the int64 numpy
restatement of tests/ccs_reference.py (the checker the GPU tests use) held to the rule's own inequality by brute force, the
committed frames against their closed form and generator, and ccs.py's ordering and text on made-up counts."""
import math
import os
import re

import numpy as np

import ccs_reference as cr
from test_analysis_cpu import ROOT, tool_module

INC = os.path.join(ROOT, "lightdock-rust_amd", "csrc", "kernels", "ccs_frames.inc")


def one_view(atoms, h):
    """atoms: (a, b, E) in one view's plane -> the reference's count."""
    a, b, E = (np.array(v, dtype=np.int64) for v in zip(*atoms))
    return cr.view_count(a, b, E, h)


# ---- the frames -------------------------------------------------------------------------------------------------

def test_frames_equal_the_closed_form_and_keep_the_tie_margin():
    table, margin = cr.frames(margin=True)
    assert table.shape == (64, 2, 3) and margin >= 1e-3              # no component within 1e-3 of a rounding tie
    assert table[0].tolist() == [[0, 1048576, 0], [-1040384, 0, 130816]]
    rows = [[int(v) for v in m.groups()] for m in re.finditer(r"^\{(-?\d+), (-?\d+), (-?\d+), (-?\d+), (-?\d+), (-?\d+)\},$", open(INC).read(), flags=re.M)]
    assert len(rows) == 64 and np.array_equal(np.array(rows).reshape(64, 2, 3), table)
    gen = tool_module(os.path.join("tools", "gen_ccs_frames"))
    again, gen_margin = gen.frames()
    assert [list(r) for r in again] == rows and gen_margin >= 1e-3
    # the axes are orthonormal and orthogonal to the surface's direction of the same index
    import sasa_reference as sr
    A, B, U = table[:, 0].astype(np.float64) / 2 ** 20, table[:, 1].astype(np.float64) / 2 ** 20, sr.U[:64].astype(np.float64) / 2 ** 20
    for x, y, want in ((A, A, 1.0), (B, B, 1.0), (A, B, 0.0), (A, U, 0.0), (B, U, 0.0)):
        assert np.abs((x * y).sum(axis=1) - want).max() < 2e-6
    assert (sr.U[:64, 2] > 0).all() and (sr.U[64:, 2] < 0).all()       # the upper hemisphere


def test_projection_rounds_half_up_and_floors_negatives():
    a, b = cr.project(np.array([[0, 1, 0], [0, -1, 0], [0, 0, 0], [1000, 2000, 3000]]))
    assert a.shape == (64, 4) and list(a[0]) == [1, -1, 0, 2000]      # view 0: A = (0, 2^20, 0)
    # B[0] = (-1040384, 0, 130816): (-1040384000 + 392448000 + 2^19) >> 20 is a floor of a negative number
    assert int(b[0, 3]) == math.floor((-1040384 * 1000 + 130816 * 3000 + 2 ** 19) / 2 ** 20) == -618


# ---- one atom ---------------------------------------------------------------------------------------------------

def test_one_atom_at_the_origin_against_brute_force():
    for h in (100, 500, 2000):
        for E in (1470, 2500, 2700, 3980):
            k = E // h + 1
            i = np.arange(-k, k + 1, dtype=np.int64)
            brute = int((((i * h) ** 2)[:, None] + ((i * h) ** 2)[None, :] <= E * E).sum())
            assert one_view([(0, 0, E)], h) == brute
            assert cr.brute_count(np.array([0]), np.array([0]), np.array([E]), h) == brute
    assert one_view([(0, 0, 2500)], 500) == 81 and one_view([(0, 0, 2499)], 500) == 69


def test_rim_points_are_counted_inclusively():
    """C (1700) with probe 0.8: E = 2500 at h = 500 has (3, 4), (5, 0) and their images exactly on the rim: 12 points."""
    assert 1700 + 800 == 2500 and (3 * 500) ** 2 + (4 * 500) ** 2 == 2500 ** 2
    def covered(E):
        j, lo, hi = cr.spans(np.array([0]), np.array([0]), np.array([E]), 500)
        return {(i, int(r)) for r, l, u in zip(j, lo, hi) for i in range(int(l), int(u) + 1)}
    at, below = covered(2500), covered(2499)
    rim = {(3, 4), (4, 3), (5, 0), (0, 5)}
    rim = {(sx * i, sy * j) for i, j in rim for sx in (1, -1) for sy in (1, -1)}
    assert len(rim) == 12 and rim <= at and not (rim & below) and at - below == rim


def test_off_origin_atoms_negative_coordinates_and_random_clumps_against_brute_force():
    rng = np.random.default_rng(7)
    for h in (100, 333, 500, 2000):
        for _ in range(6):
            n = int(rng.integers(1, 7))
            a, b = rng.integers(-9000, 9000, n), rng.integers(-9000, 9000, n)
            E = rng.choice([1470, 1520, 2550, 2700, 3980], n)
            assert cr.view_count(a, b, E, h) == cr.brute_count(a, b, E, h)
    # floor division, not truncation: a disc left of and below the origin has the count of its mirror image
    assert one_view([(-7250, -3125, 2700)], 500) == one_view([(7250, 3125, 2700)], 500)
    assert cr.ceil_div(np.array([-7, 7, -8, 0]), 4).tolist() == [-1, 2, -2, 0] and (np.array([-7, 7]) // 4).tolist() == [-2, 1]


# ---- two atoms --------------------------------------------------------------------------------------------------

def test_two_far_atoms_add_and_two_coincident_atoms_give_the_larger():
    for h in (100, 500, 2000):
        one, other = one_view([(130, -70, 2700)], h), one_view([(4000130, 5000000, 2520)], h)
        assert one_view([(130, -70, 2700), (4000130, 5000000, 2520)], h) == one + other
        assert one_view([(130, -70, 2700), (130, -70, 2520)], h) == one
        assert one_view([(130, -70, 2520), (130, -70, 2520)], h) == one_view([(130, -70, 2520)], h)
    # in three dimensions: every view of two atoms 4000 A apart along x, y and z adds up, the sum over views too
    t = np.array([[0, 0, 0], [4000000, 4000000, 4000000]])
    both = cr.counts(t, np.array([2700, 2520]), 500)
    assert np.array_equal(both, cr.counts(t[:1], np.array([2700]), 500) + cr.counts(t[1:], np.array([2520]), 500))


def test_bounds():
    E = np.array([2700, 2700])
    with np.testing.assert_raises(cr.Refused):
        cr.counts(np.array([[0, 0, 0], [10 ** 9 + 1, 0, 0]]), E, 500)
    with np.testing.assert_raises(cr.Refused):
        cr.counts(np.zeros((0, 3)), np.zeros(0), 500)
    # 16384 columns by 16384 rows is the bound itself; one more column is beyond it
    assert cr.box_points(np.array([0, 1638300 - 5400]), np.array([0, 1638300 - 5400]), E, 100) == 16384 ** 2 == cr.MAX_BOX
    assert cr.box_points(np.array([0, 1638400 - 5400]), np.array([0, 1638300 - 5400]), E, 100) == 16385 * 16384


def test_areas():
    assert float(cr.area(81)) == 81 * 0.25 and float(cr.ccs_pa(64 * 81)) == 81 * 0.25
    assert abs(float(cr.area(cr.view_count(np.array([0]), np.array([0]), np.array([2700]), 100), 0.1)) - math.pi * 2.7 ** 2) < 0.2


# ---- ccs.py's list ----------------------------------------------------------------------------------------------

def test_ordering_ties_and_text_of_rank_ccs_list():
    tool = tool_module("ccs")
    entries = [(2, 74, None, {"scoring": 31.28816735}), (0, 5, None, {"scoring": 20.5}), (7, 1, None, {"scoring": -2.5}), (3, 3, None, {"scoring": -3.0})]
    counts = np.zeros((4, 64), dtype=np.uint32)
    counts[0], counts[1], counts[2], counts[3] = 4000, 4400, 3600, 4400
    counts[0, 5], counts[0, 9] = 3000, 5000
    ccs, lo, hi = tool.areas(counts, 500)
    assert list(ccs) == [1000.0, 1100.0, 900.0, 1100.0] and list(lo) == [750.0, 1100.0, 900.0, 1100.0] and list(hi) == [1250.0, 1100.0, 900.0, 1100.0]
    assert np.array_equal(ccs, cr.ccs_pa(counts.astype(np.uint64).sum(axis=1)))
    assert tool.rank_rows(4) == [0, 1, 2, 3]
    delta = tool.deltas(ccs, 1000.0)
    assert list(delta) == [0.0, 100.0, -100.0, 100.0] and tool.rank_rows(4, delta) == [0, 1, 2, 3]      # |delta| ties keep the scoring rank
    delta = tool.deltas(ccs, 1210.0, 1.1)
    assert tool.rank_rows(4, delta) == [1, 3, 0, 2]
    assert tool.rank_text(entries, [0, 1, 2, 3], ccs, lo, hi) == (
        tool.HEADER +
        "    2        74    31.28817     1000.00    750.00   1250.00\n"
        "    0         5    20.50000     1100.00   1100.00   1100.00\n"
        "    7         1    -2.50000      900.00    900.00    900.00\n"
        "    3         3    -3.00000     1100.00   1100.00   1100.00\n")
    text = tool.rank_text(entries, [1, 3, 0, 2], ccs, lo, hi, tool.deltas(ccs, 1210.0, 1.1), 20.0)
    assert text.splitlines()[0].split() == ["Swarm", "Glowworm", "Scoring", "CCS_PA", "MinView", "MaxView", "Delta", "Delta/S"]
    assert text.splitlines()[1] == "    0         5    20.50000     1100.00   1100.00   1100.00       0.00     0.000"
    assert text.splitlines()[3] == "    2        74    31.28817     1000.00    750.00   1250.00    -110.00    -5.500"
    assert tool.rank_text([], [], ccs[:0], lo[:0], hi[:0]) == tool.HEADER
    assert tool.monomer_text("receptor", 1234.5, 1000.25, 1500.0) == "# receptor alone: CCS_PA    1234.50 A^2, views    1000.25 ..    1500.00\n"
