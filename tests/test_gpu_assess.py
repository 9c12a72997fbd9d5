"""Model quality against a reference complex on the MI355X (ld_complex_set_reference / ld_complex_assess,
lightdock-rust_amd/assess.py) against the restatement of tests/test_assess_cpu.py: `kept`, the native pairs
and the counts exactly; i-RMSD^2 within 64 eps (G_a + G_b) / n of the exact (Decimal) value and L-RMSD^2 within
128 eps (G_l,a + G_l,b) / n_l of numpy's SVD Kabsch, eps = 2^-52, no pose left out."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from test_analysis_cpu import CZY, analyse_module, read_pdb
from test_assess_cpu import (AssessRestated, assess_module, case_files, case_poses, moved, pdb_line, records, restated_case,
                             tiny_complex, write_reference)
from test_contacts_cpu import thousandths
from test_gpu_contacts import gso, perturbed_czy

pytestmark = pytest.mark.gpu

WORST = {"irmsd": 0.0, "lrmsd": 0.0}      # the worst ratios to the bounds' units (eps G / n) this session has seen


@pytest.fixture(scope="module")
def refdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("references"))


def make_complex(pkg, name):
    rec, lig, rm, lm = case_files(name)
    pkg.init(0)
    return pkg.Complex(rec, lig, rm, 0 if rm is None else 10, lm, 0 if lm is None else 10)


def fixture(pkg, name, refdir, frame=True, disturb=True):
    """The complex with the reference made from ITS OWN ld_complex_write_pdb of the reference pose, which must be the file
    the restatement made; the restatement; the poses."""
    rs, paths, poses = restated_case(name, refdir, frame, disturb)
    cx = make_complex(pkg, name)
    model = os.path.join(refdir, "%s_model.pdb" % name)
    cx.write_pdb(poses[case_poses(name)[1]][:cx.pose_len], model)
    own = write_reference(open(model).read(), cx.num_atoms(0), refdir, "%s_%d%d_gpu" % (name, frame, disturb), frame, disturb)
    assert [open(p).read() for p in own] == [open(p).read() for p in paths]
    cx.set_reference(own[0], own[1])
    return cx, rs, poses


def assert_within_bounds(got, i, m, rs):
    """Pose i of an assess() result against the restatement's measures m of it."""
    assert int(got["kept"][i]) == m["kept"]
    assert got["fnat"][i] == m["kept"] / float(len(rs.native))
    bi, bl = rs.bounds(m)
    di, dl = abs(got["irmsd"][i] ** 2 - m["irmsd2"]), abs(got["lrmsd"][i] ** 2 - m["lrmsd2"])
    WORST["irmsd"] = max(WORST["irmsd"], di / (bi / 64))
    WORST["lrmsd"] = max(WORST["lrmsd"], dl / (bl / 128))
    assert np.isfinite(got["irmsd"][i]) and np.isfinite(got["lrmsd"][i])
    assert di <= bi, (i, got["irmsd"][i] ** 2, m["irmsd2"], di / (bi / 64))
    assert dl <= bl, (i, got["lrmsd"][i] ** 2, m["lrmsd2"], dl / (bl / 128))


_MEASURES = {}


def measures_of_case(name, rs, poses):
    """The restatement's measures of every pose of a fixture, computed once."""
    if name not in _MEASURES:
        _MEASURES[name] = [rs.measures(p) for p in poses]
    return _MEASURES[name]


def check_case(pkg, name, refdir, n_poses):
    cx, rs, poses = fixture(pkg, name, refdir)
    assert len(poses) == n_poses
    assert cx.reference_counts() == rs.counts()
    assert [tuple(p) for p in cx.native_pairs().tolist()] == rs.native
    got = cx.assess(poses)
    for i, m in enumerate(measures_of_case(name, rs, poses)):
        assert_within_bounds(got, i, m, rs)
    print("%s: %d poses, worst ratios so far: i-RMSD^2 %.2f, L-RMSD^2 %.2f of eps G / n; kernels %.3f ms" %
          (name, n_poses, WORST["irmsd"], WORST["lrmsd"], cx.last_kernel_ms()))
    return cx, rs, poses, got


# ---- 1. 1czy, the 2000 final glowworms in one call ---------------------------------------------------------------

def test_1czy_every_final_glowworm_in_one_call(pkg, refdir):
    cx, rs, poses, got = check_case(pkg, "1czy", refdir, 2000)
    assert 0 < int((got["kept"] > 0).sum()) < 2000 and int(got["kept"][474]) == len(rs.native) == 25
    # the reference in the model's frame, nothing disturbed: its own pose is the reference
    cx, rs, poses = fixture(pkg, "1czy", refdir, False, False)
    assert cx.reference_counts() == rs.counts() and cx.reference_counts()["native_pairs"] == 31
    own = cx.assess(poses[474:475])
    assert own["fnat"][0] == 1.0 and 0.0 <= own["irmsd"][0] < 1e-5 and 0.0 <= own["lrmsd"][0] < 1e-5
    assert_within_bounds(own, 0, rs.measures(poses[474]), rs)


# ---- 2. smaller fixtures -----------------------------------------------------------------------------------------

def test_dna_1azp_with_p_fit_atoms(pkg, refdir):
    cx, rs, _, got = check_case(pkg, "1azp", refdir, 200)
    lines = records(case_files("1azp")[1])
    assert any(l[12:16].strip() == "P" for l, f in zip(lines, rs.lig_fit[rs.n_rec:]) if f)
    assert len(set(got["kept"].tolist())) > 2


def test_rigid_1ppe(pkg, refdir):
    cx, _, _, got = check_case(pkg, "1ppe", refdir, 120)
    assert cx.pose_len == 7 and got["kept"].max() == 43


def test_1k4c_membrane_complex(pkg, refdir):
    cx, rs, _, got = check_case(pkg, "1k4c", refdir, 32)
    assert (cx.num_atoms(0) + cx.num_atoms(1), cx.num_residues(0) + cx.num_residues(1)) == (6681, 1273)
    assert int(got["kept"][0]) == 313


def test_insertion_codes_match_as_residues_of_their_own(pkg, refdir):
    cx, rs, _, _ = check_case(pkg, "ab_icode", refdir, 48)
    ids = cx.residues(0)
    for a, b in (("H.SER.52", "H.ASP.52A"), ("H.SER.82A", "H.SER.82B")):
        ia, ib = ids.index(a), ids.index(b)
        assert rs.matched[rs.res == ia].all() and rs.matched[rs.res == ib].all()
    # the same reference without the insertion codes: those residues' records no longer match (52A) or match another's (82A/B)
    blank = os.path.join(refdir, "ab_blank_rec.pdb")
    with open(blank, "w") as f:
        f.write("".join(l[:26] + " " + l[27:] + "\n" for l in records(restated_case("ab_icode", refdir)[1][0])))
    lig = restated_case("ab_icode", refdir)[1][1]
    other = AssessRestated(*case_files("ab_icode"), blank, lig)
    assert not other.matched[other.res == ids.index("H.ASP.52A")].any() and other.counts() != rs.counts()
    cx.set_reference(blank, lig)
    assert cx.reference_counts() == other.counts() and [tuple(p) for p in cx.native_pairs().tolist()] == other.native


# ---- 4. corners on hand-made PDBs --------------------------------------------------------------------------------

STILL = np.array([[0, 0, 0, 1, 0, 0, 0.0]])


def eight_atoms(directory):
    """A chiral complex: N, CA, C, O of one receptor residue and of one ligand residue."""
    rec, lig = os.path.join(str(directory), "rec8.pdb"), os.path.join(str(directory), "lig8.pdb")
    with open(rec, "w") as f:
        f.write("".join(pdb_line(i + 1, " " + n, "ALA", "A", 5, x) for i, (n, x) in enumerate(
            (("N", (0, 0, 0)), ("CA", (1.458, 0, 0)), ("C", (2.009, 1.42, 0)), ("O", (1.6, 2.1, 0.95))))))
    with open(lig, "w") as f:
        f.write("".join(pdb_line(i + 1, " " + n, "SER", "B", 9, x) for i, (n, x) in enumerate(
            (("N", (4.1, 3.0, 2.2)), ("CA", (5.2, 3.9, 2.6)), ("C", (6.4, 3.2, 3.3)), ("O", (6.3, 2.1, 3.9))))))
    return rec, lig


def moved_reference(rec, lig, directory, name, R, t=(0.0, 0.0, 0.0)):
    paths = []
    for side, p in (("rec", rec), ("lig", lig)):
        paths.append(os.path.join(str(directory), "%s_%s.pdb" % (name, side)))
        with open(paths[-1], "w") as f:
            f.write("".join(l + "\n" for l in moved(records(p), np.array(R, dtype=float), np.array(t))))
    return paths


def test_three_fit_atoms_and_a_model_identical_to_the_reference(pkg, tmp_path):
    rec, lig = tiny_complex(tmp_path)
    pkg.init(0)
    cx = pkg.Complex(rec, lig)
    cx.set_reference(rec, lig)
    rs = AssessRestated(rec, lig, None, None, rec, lig)
    assert cx.reference_counts() == rs.counts() and cx.reference_counts()["rec_fit"] == 3
    got = cx.assess(STILL)
    assert int(got["kept"][0]) == 1 and 0.0 <= got["irmsd"][0] < 1e-5 and 0.0 <= got["lrmsd"][0] < 1e-5      # finite, not NaN
    assert_within_bounds(got, 0, rs.measures(STILL[0]), rs)
    # the native pair stepped across the cutoff in 0.0005 A: kept follows the printed thousandths
    tx = -0.002 + 0.0005 * np.arange(9)
    poses = np.repeat(STILL, 9, axis=0)
    poses[:, 0] = tx
    got = cx.assess(poses)
    printed = np.array([float("%.3f" % (3.0 + v)) for v in tx])
    assert printed.min() < 3.0 < printed.max()
    assert np.array_equal(got["kept"], (printed <= 3.0).astype(np.uint32))
    for i, p in enumerate(poses):
        assert_within_bounds(got, i, rs.measures(p), rs)


def test_identity_half_turns_and_the_mirror_image(pkg, tmp_path):
    rec, lig = eight_atoms(tmp_path)
    pkg.init(0)
    cx = pkg.Complex(rec, lig)
    frames = {"identity": np.eye(3), "x": np.diag([1, -1, -1]), "y": np.diag([-1, 1, -1]), "z": np.diag([-1, -1, 1])}
    for name, R in frames.items():
        ref = moved_reference(rec, lig, tmp_path, name, R, (3.0, -2.0, 1.0))
        cx.set_reference(*ref)
        rs = AssessRestated(rec, lig, None, None, *ref)
        assert cx.reference_counts() == rs.counts() == {"matched_rec": 4, "matched_lig": 4, "native_pairs": 1, "rec_fit": 4,
                                                        "lig_fit": 4, "interface_fit": 8}
        got = cx.assess(STILL)
        assert int(got["kept"][0]) == 1 and got["irmsd"][0] < 1e-6 and got["lrmsd"][0] < 1e-6, name
        assert_within_bounds(got, 0, rs.measures(STILL[0]), rs)
    ref = moved_reference(rec, lig, tmp_path, "mirror", np.diag([1, 1, -1]))
    cx.set_reference(*ref)
    rs = AssessRestated(rec, lig, None, None, *ref)
    got, m = cx.assess(STILL), rs.measures(STILL[0])
    assert_within_bounds(got, 0, m, rs)
    assert got["irmsd"][0] > 0.1 and m["irmsd2"] > 0.01 and int(got["kept"][0]) == 1      # a mirror image is not a fit


def test_ligand_modes_in_the_ligand_frame(pkg, refdir):
    cx, rs, poses = fixture(pkg, "1czy", refdir)
    row = gso(3)[0][0].copy()
    row[3:7] = [0.3, -0.5, 0.7, 0.4]
    row[17:27] = np.linspace(-3.0, 3.0, 10)
    got = cx.assess(row[None])
    assert_within_bounds(got, 0, rs.measures(row), rs)
    other = rs.measures(row, ligand_frame=False)                   # the scoring convention gives other numbers
    assert abs(other["lrmsd2"] - got["lrmsd"][0] ** 2) > 1e-3


# ---- 5. bits -----------------------------------------------------------------------------------------------------

def test_results_are_the_same_bits_in_any_batch(pkg, refdir):
    cx, rs, _ = fixture(pkg, "1czy", refdir)
    poses = perturbed_czy(np.random.default_rng(7), 13).reshape(2600, 27)[:2500]       # more than the 1024 slots
    whole = cx.assess(poses)
    assert np.isfinite(whole["irmsd"]).all() and np.isfinite(whole["lrmsd"]).all() and len(set(whole["kept"].tolist())) > 3
    cuts = (0, 811, 1777, 2500)                                                        # none on a slot boundary
    pieces = [cx.assess(poses[a:b]) for a, b in zip(cuts, cuts[1:])]
    back = cx.assess(poses[::-1].copy())
    for k, dtype in (("kept", np.uint32), ("irmsd", np.uint64), ("lrmsd", np.uint64)):
        assert np.array_equal(np.concatenate([p[k] for p in pieces]).view(dtype), whole[k].view(dtype))
        assert np.array_equal(back[k][::-1].copy().view(dtype), whole[k].view(dtype))
    for i in (0, 1023, 1024, 2499):
        assert_within_bounds(whole, i, rs.measures(poses[i]), rs)


# ---- 6. the PDB tie ----------------------------------------------------------------------------------------------

def test_measures_of_a_pose_are_those_of_the_pdb_file_written_for_it(pkg, refdir, tmp_path):
    cx, rs, _ = fixture(pkg, "1czy", refdir)
    poses = np.stack([gso(0)[0][0], gso(2)[0][74], gso(5)[0][100], gso(9)[0][199]])
    got = cx.assess(poses)
    for i, p in enumerate(poses):
        path = str(tmp_path / ("m%d.pdb" % i))
        cx.write_pdb(p, path)
        xyz, _ = read_pdb(path)                      # the numbers of the file's text
        assert_within_bounds(got, i, rs.measures_of(thousandths(xyz)), rs)


# ---- 7. refusals -------------------------------------------------------------------------------------------------

def test_refusals_return_invalid_and_write_nothing(pkg, refdir, tmp_path):
    lib = pkg.load_library()
    cx, rs, poses = fixture(pkg, "1czy", refdir)
    ref = restated_case("1czy", refdir)[1]
    good = np.ascontiguousarray(poses[:4])
    vp = ctypes.c_void_p

    def raw(p, stride=None, outputs=(True, True, True)):
        p = np.ascontiguousarray(p, dtype=np.float64)
        kept = np.full(len(p), 0xA5A5A5A5, dtype=np.uint32)
        l, r = np.full(len(p), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64), np.full(len(p), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        args = [a.ctypes.data_as(vp) if on else None for a, on in zip((kept, l, r), outputs)]
        status = lib.ld_complex_assess(cx._h, len(p), p.ctypes.data_as(vp), p.shape[1] if stride is None else stride, *args)
        return status, kept, l, r

    def untouched(kept, l, r):
        return (kept == 0xA5A5A5A5).all() and (l == 0xA5A5A5A5A5A5A5A5).all() and (r == 0xA5A5A5A5A5A5A5A5).all()

    def invalid(p, stride=None):
        status, kept, l, r = raw(p, stride)
        assert status == -1 and lib.ld_last_error().decode() and untouched(kept, l, r)
        if stride is None:
            with pytest.raises(pkg.LightdockError) as e:
                cx.assess(p)
            assert e.value.status == -1

    for bad in (np.nan, np.inf, -np.inf):
        p = good.copy()
        p[2, 5] = bad
        invalid(p)
    z = good.copy()
    z[1, 3:7] = 0.0
    invalid(z)
    invalid(good, stride=20)                                # stride below the pose length
    far = good.copy()
    far[3, 0] = 2100.0                                      # a used ligand atom beyond +-2000 A
    invalid(far)
    near = good.copy()
    near[3, 1] = -1900.0                                    # inside: a pose like any other
    status, kept, l, r = raw(near)
    assert status == 0 and kept[3] == 0 and np.isfinite(l.view(np.float64)).all() and l.view(np.float64)[3] > 1800.0
    ok = raw(good)
    want = cx.assess(good)
    assert ok[0] == 0 and np.array_equal(ok[1], want["kept"]) and np.array_equal(ok[2].view(np.float64), want["lrmsd"])
    # any output may be NULL; n == 0
    status, kept, l, r = raw(good, outputs=(False, True, False))
    assert status == 0 and np.array_equal(l, ok[2]) and (kept == 0xA5A5A5A5).all() and (r == 0xA5A5A5A5A5A5A5A5).all()
    assert raw(good, outputs=(False, False, False))[0] == 0
    assert lib.ld_complex_assess(cx._h, 0, None, 27, None, None, None) == 0
    empty = cx.assess(np.zeros((0, 27)))
    assert empty["kept"].shape == (0,) and empty["irmsd"].shape == (0,)

    # refusals at reference time: a message, and no reference afterwards
    rec3, lig1 = tiny_complex(tmp_path)
    two = tmp_path / "two.pdb"
    two.write_text("".join(open(rec3).read().splitlines(True)[:2] + open(rec3).read().splitlines(True)[3:]))      # N, CA, CB
    no_fit = tmp_path / "no_fit.pdb"
    no_fit.write_text(open(lig1).read().splitlines(True)[1].replace(" 30.000  30.000  30.000", "  3.000   4.000   0.000"))
    tiny = pkg.Complex(rec3, lig1)
    refusals = [(rec3, lig1, 4.999, 10.0, -1),              # no native pair
                (str(two), lig1, 5.0, 10.0, -1),            # fewer than 3 receptor fit atoms
                (rec3, str(no_fit), 5.0, 10.0, -1),         # no ligand fit atom
                (rec3, lig1, 5.0, 30.001, -1), (rec3, lig1, 0.0, 10.0, -1), (rec3, lig1, float("nan"), 10.0, -1),
                (rec3, lig1, 5.0, -1.0, -1), (rec3, lig1, 1e300, 10.0, -1),
                (str(tmp_path / "missing.pdb"), lig1, 5.0, 10.0, -3)]
    counts = np.zeros(6, dtype=np.uint32)
    for r_path, l_path, contact, interface, want_status in refusals:
        tiny.set_reference(rec3, lig1)
        assert lib.ld_complex_reference_counts(tiny._h, counts.ctypes.data_as(vp)) == 0
        status = lib.ld_complex_set_reference(tiny._h, os.fsencode(r_path), os.fsencode(l_path), ctypes.c_double(contact),
                                              ctypes.c_double(interface))
        assert status == want_status and lib.ld_last_error().decode(), (r_path, l_path, contact, interface)
        assert lib.ld_complex_reference_counts(tiny._h, counts.ctypes.data_as(vp)) == -1
        with pytest.raises(pkg.LightdockError):
            tiny.assess(STILL)
    # fewer than 3 interface fit atoms: the only residues within the interface cutoff hold two fit atoms
    tiny.set_reference(rec3, lig1, 5.0, 5.0)
    assert tiny.reference_counts()["interface_fit"] == 4
    lonely = tmp_path / "lonely.pdb"
    lonely.write_text(pdb_line(1, " N", "GLY", "A", 1, (0, 0, 0)) + pdb_line(2, " CA", "GLY", "A", 2, (-9, 0, 0)) +
                      pdb_line(3, " C", "GLY", "A", 3, (-9, 9, 20)))
    alone = pkg.Complex(str(lonely), lig1)
    with pytest.raises(pkg.LightdockError) as e:
        alone.set_reference(str(lonely), lig1, 5.0, 5.0)
    assert e.value.status == -1 and "interface" in str(e.value)
    # a complex never given a reference
    fresh = make_complex(pkg, "1czy")
    with pytest.raises(pkg.LightdockError):
        fresh.assess(good)
    with pytest.raises(pkg.LightdockError):
        fresh.native_pairs()


# ---- 8. assess.py end to end -------------------------------------------------------------------------------------

def test_assess_py_on_a_copy_of_the_1czy_run(pkg, refdir, tmp_path):
    an, am = analyse_module(), assess_module()
    cx, rs, poses = fixture(pkg, "1czy", refdir)
    ref = restated_case("1czy", refdir)[1]
    run = tmp_path / "run"
    shutil.copytree(CZY, run)
    script = os.path.join(os.path.dirname(pkg.__file__), "assess.py")

    def run_tool(*args):
        r = subprocess.run([sys.executable, script, "setup.json", "100", "--swarms", "0-9", "--reference-receptor", ref[0],
                            "--reference-ligand", ref[1]] + list(args), cwd=run, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout, open(run / "assessment.list").read()

    def restated_text(entries, measures):
        fnat = np.array([m["kept"] / float(len(rs.native)) for m in measures])
        return am.assessment_text(entries, fnat, np.sqrt([m["irmsd2"] for m in measures]), np.sqrt([m["lrmsd2"] for m in measures]))

    entries = an.ranking(range(10), 100, base=CZY)
    out, text = run_tool()
    assert len(entries) == 11 and "11 models against 25 native pairs" in out
    assert text == restated_text(entries, [rs.measures(e[2]) for e in entries])
    assert text.splitlines()[1].split()[:2] == ["2", "74"] and text.splitlines()[1].split()[3] == "1.000"
    everything = measures_of_case("1czy", rs, poses)
    scoring = np.concatenate([an.read_gso(os.path.join(CZY, "swarm_%d" % s, "gso_100.out"))[1]["scoring"] for s in range(10)])
    order = sorted(range(2000), key=lambda i: (-scoring[i], i // 200, i % 200))
    all_entries = [(i // 200, i % 200, poses[i], {"scoring": scoring[i]}) for i in order]
    out, text = run_tool("--all")
    assert "2000 models against 25 native pairs" in out
    assert text == restated_text(all_entries, [everything[i] for i in order])


# ---- 9. time -----------------------------------------------------------------------------------------------------

def test_assessment_takes_no_longer_than_the_contacts_of_the_same_poses(pkg, refdir):
    """8192 jittered 1k4c poses: the kernels of one ld_complex_assess call against those of the unchanged
    ld_complex_contacts call at 5 A on the same poses in the same process (HIP events, median of 5 after a warm-up each).
    The assessment poses a subset of the atoms (3836 of 6681) and tests only the 313 native pairs, so it has no reason to
    cost more than the full contact search.  Not measured on an MI355X yet: the test prints both times."""
    cx, rs, few = fixture(pkg, "1k4c", refdir)
    base = np.loadtxt(os.path.join(os.path.dirname(case_files("1k4c")[0]), "initial_positions_0.dat"))[:, :7]
    poses = pkg.synth.jitter(base, 8192, seed=17)
    got = cx.assess(poses)                                    # warm-up
    times = []
    for _ in range(5):
        again = cx.assess(poses)
        times.append(cx.last_kernel_ms())
    t_assess = float(np.median(times))
    assert all(np.array_equal(again[k].view(np.uint8), got[k].view(np.uint8)) for k in ("kept", "irmsd", "lrmsd"))
    for i in (0, 4097, 8191):
        assert_within_bounds(got, i, rs.measures(poses[i]), rs)
    cx.contacts(poses, packed=True)                           # warm-up
    times = []
    for _ in range(5):
        cx.contacts(poses, packed=True)
        times.append(cx.last_kernel_ms())
    t_contacts = float(np.median(times))
    print("8192 1k4c poses: T_assess %.3f ms, T_contacts %.3f ms, ratio %.2f" % (t_assess, t_contacts, t_assess / t_contacts))
    assert t_assess <= t_contacts
