"""Interface contacts on the MI355X (ld_complex_contacts, lightdock-rust_amd/filter.py): every comparison is
exact equality of bit arrays with the int64 numpy restatement of tests/test_contacts_cpu.py."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from test_analysis_cpu import CZY, analyse_module, read_pdb
from test_contacts_cpu import (GOLDEN, ContactsRestated, atom_contacts, bead_atoms, case_restated, czy_contacts_restated,
                               thousandths)

pytestmark = pytest.mark.gpu

REC = os.path.join(CZY, "lightdock_1czy_protein.pdb")
LIG = os.path.join(CZY, "lightdock_1czy_peptide.pdb")


@pytest.fixture(scope="module")
def czy(pkg):
    pkg.init(0)
    return pkg.Complex(REC, LIG, np.load(os.path.join(CZY, "lightdock_rec.nm.npy")), 10,
                       np.load(os.path.join(CZY, "lightdock_lig.nm.npy")), 10)


def case_complex(pkg, name):
    from conftest import case_paths
    c, d, rec, lig = case_paths(name)
    pkg.init(0)
    if c["use_anm"]:
        return pkg.Complex(rec, lig, np.load(os.path.join(d, "rec_nm.npy")), 10, np.load(os.path.join(d, "lig_nm.npy")), 10)
    return pkg.Complex(rec, lig)


def gso(s, case=None):
    d = CZY if case is None else os.path.join(GOLDEN, case)
    return analyse_module().read_gso(os.path.join(d, "swarm_%d" % s, "gso_100.out"))


def assert_equal_bits(got, rs, poses, cutoff=5.0):
    want_rec, want_lig = rs.batch(poses, cutoff)
    assert got["rec"].shape == want_rec.shape and got["lig"].shape == want_lig.shape
    assert np.array_equal(got["rec"], want_rec)
    assert np.array_equal(got["lig"], want_lig)


def unpack(words, n_res):
    return np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :n_res].astype(bool)


# ---- 1. the golden complexes ------------------------------------------------------------------------------------

def test_1czy_every_final_glowworm_in_one_call(czy):
    rs = czy_contacts_restated()
    assert czy.residues(0) == rs.rec_ids and czy.residues(1) == rs.lig_ids
    assert np.array_equal(czy.residue_of_atom(0), rs.rec_of) and np.array_equal(czy.residue_of_atom(1), rs.lig_of)
    poses = np.concatenate([gso(s)[0] for s in range(10)])
    got = czy.contacts(poses)
    assert_equal_bits(got, rs, poses)
    ser = rs.rec_ids.index("A.SER.467")
    assert [int(got["rec"][200 * s:200 * s + 200, ser].sum()) for s in range(10)] == [96, 0, 56, 55, 77, 106, 29, 8, 2, 3]


def test_dna_1azp_and_rigid_1ppe(pkg):
    rs = case_restated("1azp")
    cx = case_complex(pkg, "1azp")
    assert cx.residues(1) == rs.lig_ids and "B.DT.13" in rs.lig_ids and (cx.num_residues(0), cx.num_residues(1)) == (66, 16)
    poses = gso(0, "1azp")[0]
    assert len(poses) == 200
    got = cx.contacts(poses)
    assert_equal_bits(got, rs, poses)
    rec_cols = [rs.rec_ids.index(r) for r in ("A.TRP.24", "A.VAL.26", "A.ARG.42")]
    pairs = list(zip(got["rec"][:, rec_cols].sum(axis=1), got["lig"][:, rs.lig_ids.index("B.DT.13")].astype(int)))
    assert {k: pairs.count(k) for k in set(pairs)} == {(0, 1): 119, (1, 0): 13, (1, 1): 68}

    rs = case_restated("1ppe")
    cx = case_complex(pkg, "1ppe")
    assert cx.pose_len == 7
    rng = np.random.default_rng(11)
    poses = np.loadtxt(os.path.join(GOLDEN, "1ppe", "initial_positions_0.dat"))[:120, :7]
    poses[:, :3] += rng.normal(0, 1.5, (120, 3))
    got = cx.contacts(poses)
    assert_equal_bits(got, rs, poses)
    assert got["rec"].any() and not got["rec"].all()


def test_insertion_codes_are_residues_of_their_own(pkg):
    rs = case_restated("ab_icode")
    cx = case_complex(pkg, "ab_icode")
    ids = cx.residues(0)
    assert ids == rs.rec_ids and cx.residues(1) == rs.lig_ids
    six = ["H.SER.52", "H.ASP.52A", "H.MET.82", "H.SER.82A", "H.SER.82B", "H.LEU.82C"]
    assert all(ids.count(r) == 1 for r in six) and len({ids.index(r) for r in six}) == 6
    poses = np.loadtxt(os.path.join(GOLDEN, "ab_icode", "initial_positions_0.dat"))[:48]
    assert poses.shape[1] == cx.pose_len
    assert_equal_bits(cx.contacts(poses), rs, poses)


def test_1k4c_membrane_complex_and_its_beads(pkg):
    rs = case_restated("1k4c")
    cx = case_complex(pkg, "1k4c")
    assert (cx.num_atoms(0), cx.num_atoms(1), cx.num_residues(0), cx.num_residues(1)) == (3413, 3268, 845, 428)
    poses = np.loadtxt(os.path.join(GOLDEN, "1k4c", "initial_positions_0.dat"))[:32, :7]
    got = cx.contacts(poses)
    assert_equal_bits(got, rs, poses)
    mmb = np.array([r.split(".")[1] == "MMB" for r in cx.residues(0)])
    assert list(got["rec"][:10, mmb].sum(axis=1)) == [28, 33, 28, 25, 26, 34, 23, 29, 31, 31]


def test_a_complex_whose_boxes_do_not_fit_the_lds(pkg, tmp_path):
    """Two copies of 1k4c's receptor, the second 300 A away under other chain names: 1690 + 428 residues and the 54
    ligand groups are 2172 boxes of 24 B, more than the 40 KiB the kernel keeps on chip, so the boxes live in the workspace."""
    from conftest import case_paths
    _, d, rec, lig = case_paths("1k4c")
    lines = [l for l in open(rec) if l.startswith(("ATOM  ", "HETATM"))]
    far = [l[:21] + chr(ord(l[21]) + 10) + l[22:30] + "%8.3f" % (float(l[30:38]) + 300.0) + l[38:] for l in lines]
    twice = tmp_path / "twice.pdb"
    twice.write_text("".join(lines + far))
    pkg.init(0)
    cx = pkg.Complex(str(twice), lig)
    rs = ContactsRestated(str(twice), lig)
    assert cx.num_residues(0) == 1690 and cx.residues(0) == rs.rec_ids
    poses = np.loadtxt(os.path.join(d, "initial_positions_0.dat"))[:6, :7]
    poses[3:, 0] += 300.0                       # three poses at the copy
    got = cx.contacts(poses)
    assert_equal_bits(got, rs, poses)
    assert got["rec"][:3, :845].any() and not got["rec"][:3, 845:].any() and got["rec"][3:, 845:].any()
    assert np.array_equal(got["rec"][:3, :845], case_complex(pkg, "1k4c").contacts(poses[:3])["rec"])


# ---- 2. knife edges ---------------------------------------------------------------------------------------------

def pdb_line(serial, resname, chain, seq, xyz):
    return "ATOM  %5d  CA  %3s %1s%4d    %8.3f%8.3f%8.3f  1.00  0.00           C\n" % ((serial, resname, chain, seq) + tuple(xyz))


def test_knife_edge_by_construction(pkg, tmp_path):
    """Receptor atoms at the origin and at (50, 0, 0); ligand atoms at the origin and, 3-4-5 from the second receptor
    atom, at (53, 4, 0).  The translation steps the first ligand atom along x across 4.998 ... 5.002 in 0.0005 A."""
    rec, lig = tmp_path / "rec.pdb", tmp_path / "lig.pdb"
    rec.write_text(pdb_line(1, "GLY", "A", 1, (0, 0, 0)) + pdb_line(2, "ALA", "A", 2, (50, 0, 0)))
    lig.write_text(pdb_line(1, "SER", "B", 1, (0, 0, 0)) + pdb_line(2, "THR", "B", 2, (53, 4, 0)))
    pkg.init(0)
    cx = pkg.Complex(str(rec), str(lig))
    rs = ContactsRestated(str(rec), str(lig))
    assert cx.residues(0) == ["A.GLY.1", "A.ALA.2"] and cx.residues(1) == ["B.SER.1", "B.THR.2"]
    tx = 4.998 + 0.0005 * np.arange(9)
    poses = np.zeros((9, 7))
    poses[:, 0] = tx
    poses[:, 3] = 1.0
    got = cx.contacts(poses, 5.0)
    assert_equal_bits(got, rs, poses)
    printed = np.array([float("%.3f" % v) for v in tx])
    assert printed.min() < 5.0 < printed.max()
    assert np.array_equal(got["rec"][:, 0], printed <= 5.0) and np.array_equal(got["lig"][:, 0], printed <= 5.0)
    assert not got["rec"][:, 1].any() and not got["lig"][:, 1].any()
    still = np.array([[0, 0, 0, 1, 0, 0, 0.0]])
    at5, below = cx.contacts(still, 5.0), cx.contacts(still, 4.999)
    assert list(at5["rec"][0]) == [True, True] and list(at5["lig"][0]) == [True, True]       # 3-4-5: 25 000 000 <= 5000^2
    assert list(below["rec"][0]) == [True, False] and list(below["lig"][0]) == [True, False]


def test_ligand_modes_in_the_ligand_frame(czy):
    rs = czy_contacts_restated()
    row = gso(3)[0][0].copy()
    row[3:7] = [0.3, -0.5, 0.7, 0.4]
    row[17:27] = np.linspace(-3.0, 3.0, 10)
    got = czy.contacts(row[None])
    rec, lig = rs.contacts(row)
    other = rs.contacts(row, ligand_frame=False)
    assert np.array_equal(got["rec"][0], rec) and np.array_equal(got["lig"][0], lig)
    assert rec.any() and not np.array_equal(rec, other[0])      # the scoring convention gives other bits


# ---- 3. cutoffs -------------------------------------------------------------------------------------------------

def test_cutoffs_monotone_and_bounds(pkg, czy):
    rs = czy_contacts_restated()
    poses = gso(5)[0]
    last = None
    for cutoff in (0.001, 4.0, 5.0, 12.5, 30.0):
        got = czy.contacts(poses, cutoff)
        assert_equal_bits(got, rs, poses, cutoff)
        if last is not None:
            assert not (last["rec"] & ~got["rec"]).any() and not (last["lig"] & ~got["lig"]).any()
        last = got
    assert last["lig"].all() and not czy.contacts(poses, 0.001)["rec"].any()
    lib = pkg.load_library()
    p = np.ascontiguousarray(poses[:4])
    for bad in (30.001, 0.0, -1.0, float("nan"), 1e300):
        rec = np.full((4, 6), 0xA5A5A5A5, dtype=np.uint32)
        lig = np.full((4, 1), 0xA5A5A5A5, dtype=np.uint32)
        status = lib.ld_complex_contacts(czy._h, 4, p.ctypes.data_as(ctypes.c_void_p), p.shape[1], ctypes.c_double(bad),
                                         rec.ctypes.data_as(ctypes.c_void_p), lig.ctypes.data_as(ctypes.c_void_p))
        assert status == -1 and lib.ld_last_error().decode()
        assert (rec == 0xA5A5A5A5).all() and (lig == 0xA5A5A5A5).all()
        with pytest.raises(pkg.LightdockError):
            czy.contacts(poses[:4], bad)


# ---- 4. the PDB tie ---------------------------------------------------------------------------------------------

def test_contacts_of_a_pose_are_those_of_the_pdb_file_written_for_it(czy, tmp_path):
    rs = czy_contacts_restated()
    poses = np.stack([gso(0)[0][0], gso(3)[0][17], gso(5)[0][100], gso(9)[0][199]])
    got = czy.contacts(poses)
    assert got["rec"].any()
    for i, p in enumerate(poses):
        path = str(tmp_path / ("m%d.pdb" % i))
        czy.write_pdb(p, path)
        xyz, _ = read_pdb(path)                      # the numbers of the file's text
        rec, lig = rs.residue_bits(xyz)
        assert np.array_equal(got["rec"][i], rec) and np.array_equal(got["lig"][i], lig)


# ---- 5. every glowworm of 1024 swarms ---------------------------------------------------------------------------

def perturbed_czy(rng, n_swarms):
    base = np.stack([gso(s)[0] for s in range(10)])
    poses = base[np.arange(n_swarms) % 10].copy()
    poses[:, :, :3] += rng.normal(0, 1.0, poses[:, :, :3].shape)
    q = poses[:, :, 3:7] + rng.normal(0, 0.05, poses[:, :, 3:7].shape)
    poses[:, :, 3:7] = q / np.linalg.norm(q, axis=2)[:, :, None]
    poses[:, :, 7:] += rng.normal(0, 0.1, poses[:, :, 7:].shape)
    return poses


def test_1024_swarms_in_one_call(czy):
    rs = czy_contacts_restated()
    poses = perturbed_czy(np.random.default_rng(5), 1024).reshape(204800, 27)
    words = czy.contacts(poses, packed=True)
    print("1024 x 200 1czy poses: contacts kernels %.3f ms" % czy.last_kernel_ms())
    assert words["rec"].shape == (204800, 6) and words["lig"].shape == (204800, 1)
    # at most 1024 workgroups a launch: every workgroup reused its workspace slot for 200 poses
    assert not (words["rec"][:, 5] >> np.uint32(168 - 160)).any() and not (words["lig"][:, 0] >> np.uint32(7)).any()
    rec, lig = unpack(words["rec"], 168), unpack(words["lig"], 7)
    assert np.array_equal(rec.any(axis=1), lig.any(axis=1))
    assert 0 < rec.any(axis=1).sum() < 204800
    for k in (0, 1, 9, 137, 500, 511, 777, 1023):
        sl = slice(200 * k, 200 * k + 200)
        assert_equal_bits({"rec": rec[sl], "lig": lig[sl]}, rs, poses[sl])
    cuts = (0, 70001, 140003, 204800)        # three pieces, none on a chunk boundary
    pieces = [czy.contacts(poses[a:b], packed=True) for a, b in zip(cuts, cuts[1:])]
    assert np.array_equal(np.concatenate([p["rec"] for p in pieces]), words["rec"])
    assert np.array_equal(np.concatenate([p["lig"] for p in pieces]), words["lig"])


# ---- 6. errors --------------------------------------------------------------------------------------------------

def test_errors_return_invalid_and_write_nothing(pkg, czy):
    lib = pkg.load_library()
    good = gso(0)[0][:4]

    def raw(p, stride=None):
        p = np.ascontiguousarray(p, dtype=np.float64)
        rec = np.full((len(p), 6), 0xA5A5A5A5, dtype=np.uint32)
        lig = np.full((len(p), 1), 0xA5A5A5A5, dtype=np.uint32)
        status = lib.ld_complex_contacts(czy._h, len(p), p.ctypes.data_as(ctypes.c_void_p), p.shape[1] if stride is None else stride,
                                         ctypes.c_double(5.0), rec.ctypes.data_as(ctypes.c_void_p), lig.ctypes.data_as(ctypes.c_void_p))
        return status, rec, lig

    def invalid(p, stride=None):
        status, rec, lig = raw(p, stride)
        assert status == -1 and lib.ld_last_error().decode()
        assert (rec == 0xA5A5A5A5).all() and (lig == 0xA5A5A5A5).all()
        with pytest.raises(pkg.LightdockError) as e:
            czy.contacts(p)
        assert e.value.status == -1

    for bad in (np.nan, np.inf, -np.inf):
        p = good.copy()
        p[2, 5] = bad
        invalid(p)
    z = good.copy()
    z[1, 3:7] = 0.0
    invalid(z)
    invalid(good[:, :20])                                   # stride below the pose length
    far = good.copy()
    far[3, 0] = 1.1e6                                       # beyond the coordinate bound
    invalid(far)
    near = good.copy()
    near[3, 1] = -0.9e6                                     # inside it: a pose like any other, in contact with nothing
    status, rec, lig = raw(near)
    assert status == 0 and not rec[3].any() and not lig[3].any()
    assert np.array_equal(unpack(rec[:3], 168), czy.contacts(good[:3])["rec"])
    ok = raw(good)
    assert ok[0] == 0 and not (ok[1] == 0xA5A5A5A5).all()
    # one output or none
    p = np.ascontiguousarray(good)
    lig = np.zeros((4, 1), dtype=np.uint32)
    assert lib.ld_complex_contacts(czy._h, 4, p.ctypes.data_as(ctypes.c_void_p), 27, ctypes.c_double(5.0), None,
                                   lig.ctypes.data_as(ctypes.c_void_p)) == 0
    assert np.array_equal(lig, ok[2])
    assert lib.ld_complex_contacts(czy._h, 4, p.ctypes.data_as(ctypes.c_void_p), 27, ctypes.c_double(5.0), None, None) == 0
    empty = czy.contacts(np.zeros((0, 27)))
    assert empty["rec"].shape == (0, 168) and empty["lig"].shape == (0, 7)
    # residue ids
    buf = ctypes.create_string_buffer(64)
    assert lib.ld_complex_residue_id(czy._h, 0, 0, buf, 64) == 0 and buf.value.decode() == czy.residues(0)[0]
    n = len(buf.value)
    short = ctypes.create_string_buffer(b"#" * 63, 64)
    assert lib.ld_complex_residue_id(czy._h, 0, 0, short, n) == -1 and short.value == b"#" * 63     # no room for the NUL
    assert lib.ld_complex_residue_id(czy._h, 0, 0, short, n + 1) == 0 and short.value == buf.value
    assert lib.ld_complex_residue_id(czy._h, 0, 168, buf, 64) == -1
    assert lib.ld_complex_residue_id(czy._h, 2, 0, buf, 64) == -1 and lib.ld_complex_residue_id(czy._h, -1, 0, buf, 64) == -1
    assert czy.num_residues(2) == 0 and czy.num_residues(-1) == 0
    with pytest.raises(pkg.LightdockError):
        czy.residues(2)
    with pytest.raises(pkg.LightdockError):
        czy.residue_of_atom(2)


# ---- 7. filter.py end to end ------------------------------------------------------------------------------------

def run_filter(pkg, run, *args):
    script = os.path.join(os.path.dirname(pkg.__file__), "filter.py")
    r = subprocess.run([sys.executable, script] + list(args), cwd=run, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout, open(os.path.join(run, "filtered", "rank_filtered.list")).read().splitlines()


def test_filter_keeps_the_models_that_touch_the_restraint_of_1czy(pkg, czy, tmp_path):
    an = analyse_module()
    run = tmp_path / "run"
    shutil.copytree(CZY, run)
    out, lines = run_filter(pkg, run, "setup.json", "100", "--swarms", "0-9", "--write-pdb")
    entries = an.ranking(range(10), 100, base=CZY)
    assert len(entries) == 11 and "6 of 11 models kept" in out
    assert lines[1:] == ["%5d %9d %11.5f %8.3f %8.3f %7d" % (s, g, c["scoring"], 1.0, -1.0, 0) for s, g, _, c in entries[:6]]
    assert sorted(os.listdir(run / "filtered")) == sorted(["rank_filtered.list"] + ["swarm_%d_%d.pdb" % e[:2] for e in entries[:6]])
    for s, g, pose, _ in entries[:6]:
        want = str(tmp_path / "want.pdb")
        czy.write_pdb(pose[:27], want)
        assert (run / "filtered" / ("swarm_%d_%d.pdb" % (s, g))).read_bytes() == open(want, "rb").read()
    out, lines = run_filter(pkg, run, "setup.json", "100", "--swarms", "0-9", "--all", "--restraints", "restraints.list")
    assert "432 of 2000 models kept" in out and len(lines) == 433
    scores = [float(l.split()[2]) for l in lines[1:]]
    assert scores == sorted(scores, reverse=True)
    with open(run / "bad.list", "w") as f:
        f.write("R A.SER.467 A\nR A.TRP.9999\n")
    script = os.path.join(os.path.dirname(pkg.__file__), "filter.py")
    r = subprocess.run([sys.executable, script, "setup.json", "100", "--swarms", "0-9", "--restraints", "bad.list"], cwd=run,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "A.TRP.9999" in r.stderr


def test_filter_drops_the_models_in_the_membrane_of_1k4c(pkg, tmp_path):
    import json
    rs = case_restated("1k4c")
    d = os.path.join(GOLDEN, "1k4c")
    setup = json.load(open(os.path.join(d, "setup.json")))
    assert setup["swarms"] == 101 and not setup["receptor_restraints"]["active"] + setup["receptor_restraints"]["passive"]
    wanted = setup["ligand_restraints"]["active"] + setup["ligand_restraints"]["passive"]
    poses, cols = gso(0, "1k4c")
    poses = poses[:, :7]
    assert len(poses) == 200
    beads_at, n_rec = bead_atoms(rs), len(rs.rec)
    lig_at = [np.flatnonzero(rs.lig_of == rs.lig_ids.index(r)) for r in wanted]
    beads, frac = [], []
    for p in poses:                      # beads x ligand atoms, receptor atoms x restraint atoms: not all pairs
        t = thousandths(rs.pose(p))
        beads.append(int(atom_contacts(t[beads_at], t[n_rec:], 5.0).any(axis=1).sum()))
        frac.append(sum(bool(atom_contacts(t[:n_rec], t[n_rec + a], 5.0).any()) for a in lig_at) / float(len(wanted)))
    beads, frac = np.array(beads), np.array(frac)
    N = int(np.median(beads))
    print("1k4c swarm 0: beads %d ... %d, median %d; ligand restraint fraction %.2f ... %.2f" %
          (beads.min(), beads.max(), N, frac.min(), frac.max()))
    assert 0 < (beads <= N).sum() < 200
    keep = (frac >= 0.4) & (beads <= N)
    order = sorted(range(200), key=lambda g: (-cols["scoring"][g], g))
    run = tmp_path / "run"
    shutil.copytree(d, run)
    out, lines = run_filter(pkg, run, "setup.json", "100", "--all", "--swarms", "0", "--max-beads", str(N))
    assert "%d of 200 models kept" % keep.sum() in out
    assert lines[1:] == ["%5d %9d %11.5f %8.3f %8.3f %7d" % (0, g, cols["scoring"][g], -1.0, frac[g], beads[g]) for g in order if keep[g]]


# ---- 8. time ----------------------------------------------------------------------------------------------------

def test_contacts_take_no_more_than_eight_times_the_dfire_scorer(pkg, table):
    """8192 1k4c poses: the kernels of one contacts call at 5 A against the DFIRE scorer's device-batch call on the same
    poses (HIP events, median of 5 after a warm-up each).  All pairs would be >= 19 ms of pure issue, ~17 x the scorer:
    the gate is half of that.  Measured 2026-10-16 on one MI355X: T_contacts 1.46 ms, T_dfire 1.23 ms, ratio 1.18."""
    torch = pytest.importorskip("torch")
    from conftest import case_paths
    _, d, rec, lig = case_paths("1k4c")
    pkg.init(0)
    base = np.loadtxt(os.path.join(d, "initial_positions_0.dat"))[:, :7]
    poses = pkg.synth.jitter(base, 8192, seed=17)
    cx = pkg.Complex(rec, lig)
    got = cx.contacts(poses)                                  # warm-up
    times = []
    for _ in range(5):
        again = cx.contacts(poses, packed=True)
        times.append(cx.last_kernel_ms())
    t_contacts = float(np.median(times))
    assert np.array_equal(unpack(again["rec"], 845), got["rec"])
    rs = case_restated("1k4c")
    for i in (0, 4097, 8191):
        want = rs.contacts(poses[i])
        assert np.array_equal(got["rec"][i], want[0]) and np.array_equal(got["lig"][i], want[1])

    scorer = pkg.Scorer.from_pdb("dfire", rec, lig, potential=table)
    dev = torch.device("cuda:0")
    d_poses = torch.from_numpy(poses).to(dev)
    d_out = torch.zeros(8192, dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(device=dev)        # a stream of torch's own: the NULL stream would mean the scorer's own
    torch.cuda.synchronize()
    scorer.set_stream(stream.cuda_stream)
    times = []
    for k in range(6):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        scorer.energy_batch_device(8192, d_poses.data_ptr(), 7, d_out.data_ptr())
        t1.record(stream)
        torch.cuda.synchronize()
        if k:
            times.append(t0.elapsed_time(t1))
    scorer.set_stream(0)
    t_dfire = float(np.median(times))
    assert np.isfinite(d_out.cpu().numpy()).all()
    print("8192 1k4c poses: T_contacts %.3f ms, T_dfire %.3f ms, ratio %.2f" % (t_contacts, t_dfire, t_contacts / t_dfire))
    assert t_contacts <= 8.0 * t_dfire
