"""Model quality on the MI355X at its edges: ld_complex_set_reference / ld_complex_assess (complex_assess_sums and
complex_assess_solve, kernels/assess.hip; assess_horn, kernels/assess.hpp) on every case of tests/assess_edges.py, each of
which tests/test_assess_edges_cpu.py shows to be what it says.  Per case: reference_counts() and native_pairs() equal to the
restatement (test_assess_cpu.AssessRestated), `kept` equal, fnat == kept / n_native, results finite, i-RMSD^2 within
64 eps (G_a + G_b) / n and L-RMSD^2 within 128 eps (G_l,a + G_l,b) / n_l (1 + kappa) of the 60-digit reference
(assess_edges.reference_measures, where the bounds are derived); at kappa = inf L-RMSD^2 is only held to be finite, non-negative
and at most (sqrt(G_l,a / n_l) + sqrt(G_l,b / n_l))^2.  No case and no pose is left out.

Measured on an MI355X, 2026-10-20, all 41 tests of this file in 5 s: the worst |error| over every case was 3.12 of eps G / n
for i-RMSD^2 (bound 64; a tile case) and 0.72 of eps G / n_l (1 + kappa) for L-RMSD^2 (bound 128; 180.001 degrees about
(1, 2, 2)); on the kappa ladder L-RMSD^2 stayed within 0.013 of that unit at every rung, kappa 81 to 8.1e7; the unspecified
L-RMSD^2 of the collinear receptor came to 0.026 of its cap.  Each test prints its own worst ratios.

What a wrong kernel fails (each tried on an MI355X, the mutated library against this file).  The tile walk one short (ta + 1 <
pr.y: a last tile of one atom is skipped): every case whose residues hold 1, 9 or 17 atoms -- the four corner tests, the slot
test, the solver cases, whose residues are single atoms.  The eighth column of a tile never tested ((lane & 7) % 7): the
corners first_last and last_last.  The last native pair left out: the pair counts 7, 8, 9 and 17 and C = 30000.  The bound as
|c| < 2000000: the coordinate-bound test alone.  clamped_abs without its clamp: the aliasing distances and C = 30000.
On the host build of assess.hpp (it is host code too): three Jacobi sweeps for ten, or the eigenvector of another diagonal
entry than the largest, miss the bounds by factors of 1e3 to 1e15 on the ladder, the half turns and the mirror family; the
high word of assess_to_double dropped is caught by the 4096-atom case alone."""
import ctypes

import numpy as np
import pytest

import assess_edges as ae

pytestmark = pytest.mark.gpu

WORST = {"irmsd": 0.0, "lrmsd": 0.0, "cap": 0.0}      # the worst ratios to the bounds' units this session has seen


@pytest.fixture(scope="module")
def directory(tmp_path_factory):
    return str(tmp_path_factory.mktemp("assess_edges"))


def check_row(got, i, m, b):
    """Row i of an assess() result against the reference's measures m of that pose."""
    name = b.case.name
    assert int(got["kept"][i]) == m["kept"], (name, i, int(got["kept"][i]), m["kept"])
    assert got["fnat"][i] == m["kept"] / float(len(b.rs.native)), (name, i)
    assert np.isfinite(got["irmsd"][i]) and np.isfinite(got["lrmsd"][i]) and got["irmsd"][i] >= 0.0 and got["lrmsd"][i] >= 0.0, (name, i)
    bi, bl = ae.bounds(m)
    di = abs(got["irmsd"][i] ** 2 - m["irmsd2"])
    WORST["irmsd"] = max(WORST["irmsd"], di / (bi / 64))
    assert di <= bi, (name, i, got["irmsd"][i] ** 2, m["irmsd2"], di / (bi / 64))
    if bl is None:
        WORST["cap"] = max(WORST["cap"], got["lrmsd"][i] ** 2 / ae.lrmsd_cap(m))
        assert got["lrmsd"][i] ** 2 <= ae.lrmsd_cap(m), (name, i, got["lrmsd"][i] ** 2, ae.lrmsd_cap(m))
        return
    dl = abs(got["lrmsd"][i] ** 2 - m["lrmsd2"])
    WORST["lrmsd"] = max(WORST["lrmsd"], dl / (bl / 128))
    assert dl <= bl, (name, i, got["lrmsd"][i] ** 2, m["lrmsd2"], dl / (bl / 128), m["kappa"])


def run_case(pkg, case, directory):
    """The case through Complex, set_reference and one assess() of all its poses, every row checked -> (complex, Built, result)."""
    b = ae.built(case, directory)
    pkg.init(0)
    cx = pkg.Complex(b.paths[0], b.paths[1])
    cx.set_reference(b.paths[2], b.paths[3], case.C / 1000.0, case.I / 1000.0)
    assert cx.reference_counts() == b.rs.counts(), case.name
    assert [tuple(p) for p in cx.native_pairs().tolist()] == b.rs.native, case.name
    got = cx.assess(case.rows)
    assert len(got["kept"]) == len(case.poses)
    for i in range(len(case.poses)):
        check_row(got, i, b.measures(i), b)
    return cx, b, got


def report(what):
    print("%s: worst ratios so far: i-RMSD^2 %.3f of eps G / n, L-RMSD^2 %.3f of eps G / n_l (1 + kappa), unspecified L-RMSD^2 %.3f of its cap"
          % (what, WORST["irmsd"], WORST["lrmsd"], WORST["cap"]))


# ---- the solver --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ae.solver_cases(), ids=lambda c: c.name)
def test_solver_cases(pkg, directory, case):
    """The kappa ladder down to a collinear receptor, a collinear interface, S = 0, half turns about no axis, 180 +- 0.001
    degrees, 1e-6 rad, mirror images with closing singular values, a perfect fit over +-1900 A, the corner of the cube."""
    cx, b, got = run_case(pkg, case, directory)
    m = b.measures(0)
    if case.expect.get("zero_s"):
        assert abs(got["irmsd"][0] ** 2 - (m["ga"] + m["gb"]) / m["n_int"]) <= ae.bounds(m)[0]
    if case.expect.get("perfect"):
        assert got["irmsd"][0] ** 2 <= ae.bounds(m)[0] and got["lrmsd"][0] ** 2 <= ae.bounds(m)[1] and int(got["kept"][0]) == 12
    if case.expect.get("mirror"):
        assert got["irmsd"][0] > 1.0                                    # a mirror image is not a fit
    print("%s: kappa %.4g, i-RMSD^2 %.17g (reference %.17g), L-RMSD^2 %.17g (reference %.17g)"
          % (case.name, m["kappa"], got["irmsd"][0] ** 2, m["irmsd2"], got["lrmsd"][0] ** 2, m["lrmsd2"]))
    report(case.name)


def test_4096_fit_atoms_a_side_over_the_whole_cube(pkg, directory):
    """Sums near 2^55 and n * sum near 2^67 through the __int128 centring and assess_to_double."""
    cx, b, got = run_case(pkg, ae.spread_case(), directory)
    assert 1.0 < got["irmsd"][0] < 3.0 and 1.5 < got["lrmsd"][0] < 2.5
    report("spread_4096")


# ---- the sums kernel ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("corner", ae.TILE_CORNERS)
def test_the_sole_contact_at_each_corner_of_the_residue_pair(pkg, directory, corner):
    """Residues of 1, 7, 8, 9, 16, 17 and 24 matched atoms against each other; the only atom pair in contact is (first or last,
    first or last), at exactly C in pose 0 and at 3001, 4000, 0 in pose 1."""
    for case in ae.tile_cases(corner):
        cx, b, got = run_case(pkg, case, directory)
        assert got["kept"].tolist() == [1, 0] and got["fnat"].tolist() == [1.0, 0.0], case.name
    report("tiles, " + corner)


@pytest.mark.parametrize("count", ae.PAIR_COUNTS)
def test_native_pairs_dealt_to_the_waves(pkg, directory, count):
    """1, 7, 8, 9 and 17 native pairs over 8 waves: all kept, none, the even ones, the odd ones."""
    case = ae.pairs_case(count)
    cx, b, got = run_case(pkg, case, directory)
    assert got["kept"].tolist() == case.expect["kept"]
    report("%d native pairs" % count)


@pytest.mark.parametrize("C", (1, 30000))
def test_the_smallest_and_the_largest_cutoff(pkg, directory, C):
    case = ae.cutoff_case(C)
    cx, b, got = run_case(pkg, case, directory)
    extra = len(b.rs.native) - 1
    assert (got["kept"].astype(int) - extra).tolist() == case.expect["kept_of_pair"]       # C, 0, 0; C, 1, 0; C + 1, 0, 0; C - 1, 0, 0
    report("C = %d" % C)


def test_distances_whose_32_bit_square_is_under_the_cutoff(pkg, directory):
    case = ae.aliasing_case()
    cx, b, got = run_case(pkg, case, directory)
    assert got["kept"].tolist() == [1, 0, 0, 0, 0]
    print("distances on x: %s; on the three axes: %s" % case.expect["distances"])
    report("aliasing")


@pytest.mark.parametrize("counts", ae.USED_COUNTS, ids=lambda c: "%d_%d" % c)
def test_used_atom_counts_around_the_workgroup_size(pkg, directory, counts):
    """3 ... 513 used atoms against 1, 64, 513, the five kinds of atom interleaved in file order."""
    cx, b, got = run_case(pkg, ae.used_case(*counts), directory)
    assert got["irmsd"].min() > 0.03
    report("used atoms %d, %d" % counts)


def test_slots_reused_by_more_poses_than_there_are(pkg, directory):
    """1030 poses alternating between in and out on the last lane of the last tile: every row right, the same bits a second time
    and for every pose of the same translation."""
    case = ae.slot_case()
    cx, b, got = run_case(pkg, case, directory)
    assert got["kept"].tolist() == [1, 0] * 515
    again = cx.assess(case.rows)
    for key, dtype in (("kept", np.uint32), ("irmsd", np.uint64), ("lrmsd", np.uint64)):
        assert np.array_equal(again[key].view(dtype), got[key].view(dtype)), key
        assert np.array_equal(got[key].view(dtype), np.tile(got[key][:2].view(dtype), 515)), key
    report("1030 poses")


# ---- the coordinate bound ----------------------------------------------------------------------------------------

def test_the_bound_at_the_thousandth_counts_used_atoms_only(pkg, directory):
    """A used ligand atom posed to exactly +-2000.000 A is measured like any other; at +-2000.0006 A (which prints as 2000.001) the
    call is refused with status -1 and nothing is written; the unmatched atom at 5000 A and the matched but unused one at
    4000 A in the ligand's file refuse nothing."""
    case = ae.bound_case()
    cx, b, got = run_case(pkg, case, directory)
    assert got["kept"].tolist() == [0, 0, 0, 0, 1] and got["lrmsd"][:4].min() > 1900.0
    near = cx.assess(ae.ACCEPTED_ROWS)                       # 2000.0004 prints as 2000.000: the same thousandths, the same bits
    for key, dtype in (("kept", np.uint32), ("irmsd", np.uint64), ("lrmsd", np.uint64)):
        assert np.array_equal(near[key].view(dtype), got[key][[0, 3]].view(dtype)), key
    lib, vp = pkg.load_library(), ctypes.c_void_p

    def raw(rows):
        p = np.ascontiguousarray(rows, dtype=np.float64)
        kept = np.full(len(p), 0xA5A5A5A5, dtype=np.uint32)
        l, r = np.full(len(p), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64), np.full(len(p), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        status = lib.ld_complex_assess(cx._h, len(p), p.ctypes.data_as(vp), p.shape[1], kept.ctypes.data_as(vp), l.ctypes.data_as(vp),
                                       r.ctypes.data_as(vp))
        return status, kept, l, r

    good = case.rows
    for bad in ae.REFUSED_ROWS:
        for rows in (bad[None], np.concatenate([good[:2], bad[None], good[2:]])):
            status, kept, l, r = raw(rows)
            assert status == -1 and "2000" in lib.ld_last_error().decode()
            assert (kept == 0xA5A5A5A5).all() and (l == 0xA5A5A5A5A5A5A5A5).all() and (r == 0xA5A5A5A5A5A5A5A5).all()
            with pytest.raises(pkg.LightdockError) as e:
                cx.assess(rows)
            assert e.value.status == -1
    status, kept, l, r = raw(good)                           # and the complex still serves: the rows above, bit for bit
    assert status == 0 and np.array_equal(kept, got["kept"]) and np.array_equal(l.view(np.float64), got["lrmsd"])
    assert np.array_equal(r.view(np.float64), got["irmsd"])
    report("bound")
