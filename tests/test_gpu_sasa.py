"""The solvent-accessible surface on the MI355X (ld_complex_sasa, lightdock-rust_amd/interface.py): every
comparison is exact equality of integer arrays with the int64 numpy restatement of tests/sasa_reference.py."""
import ctypes
import itertools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import sasa_reference as sr
from test_analysis_cpu import CZY, analyse_module, read_pdb, tool_module
from test_contacts_cpu import GOLDEN, thousandths
from test_gpu_contacts import REC, LIG, case_complex, gso, perturbed_czy

pytestmark = pytest.mark.gpu

FILL = 0xA5


@pytest.fixture(scope="module")
def czy(pkg):
    pkg.init(0)
    return pkg.Complex(REC, LIG, np.load(os.path.join(CZY, "lightdock_rec.nm.npy")), 10,
                       np.load(os.path.join(CZY, "lightdock_lig.nm.npy")), 10)


@pytest.fixture(scope="module")
def czy_rs():
    return sr.czy_sasa()


def assert_equal(got, rs, poses, probe=1.4):
    sums, free, bound = rs.batch(poses, probe)
    assert got["sums"].dtype == np.uint64 and got["free"].dtype == np.uint8 and got["bound"].dtype == np.uint8
    assert got["sums"].shape == sums.shape and got["free"].shape == free.shape and got["bound"].shape == bound.shape
    assert np.array_equal(got["free"], free)
    assert np.array_equal(got["bound"], bound)
    assert np.array_equal(got["sums"], sums)
    return sums, free, bound


def atom(serial, name, resname, chain, seq, xyz, element, hetatm=False):
    """A full 80-column record; element "" leaves columns 77-78 blank."""
    return "%-6s%5d %-4s %3s %1s%4d    %8.3f%8.3f%8.3f  1.00  0.00          %2s  \n" % (
        ("HETATM" if hetatm else "ATOM", serial, name, resname, chain, seq) + tuple(xyz) + (element,))


def pair_of_files(tmp_path, rec_text, lig_text, tag=""):
    rec, lig = tmp_path / ("rec%s.pdb" % tag), tmp_path / ("lig%s.pdb" % tag)
    rec.write_text(rec_text)
    lig.write_text(lig_text)
    return str(rec), str(lig)


def rigid(n, tx=None):
    poses = np.zeros((n, 7))
    poses[:, 3] = 1.0
    if tx is not None:
        poses[:, 0] = tx
    return poses


# ---- 1. knife edges ---------------------------------------------------------------------------------------------

def test_knife_edges_of_two_atoms(pkg, tmp_path):
    """A one-atom receptor and a one-atom ligand, both at the origin of their files; the pose moves the ligand along x."""
    pkg.init(0)
    tx = np.concatenate([2.990 + 0.0005 * np.arange(41), [0.0, 0.001, 6.198, 6.199, 6.200, 6.201]])
    poses = rigid(len(tx), tx)
    printed = thousandths(tx)
    assert printed[:41].min() == 2990 and printed[:41].max() == 3010
    for tag, element, want in (("cc", "C", {0: (69, 69), 1: (66, 64), 3000: (95, 95), 6198: (128, 128), 6199: (128, 128),
                                            6200: (128, 128), 6201: (128, 128)}), ("co", "O", {3000: (99, 92)})):
        rec, lig = pair_of_files(tmp_path, atom(1, "C", "GLY", "A", 1, (0, 0, 0), "C"), atom(1, element, "GLY", "B", 1, (0, 0, 0), element), tag)
        cx, rs = pkg.Complex(rec, lig), sr.SasaRestated(rec, lig)
        got = cx.sasa(poses, atoms=True)
        assert_equal(got, rs, poses)
        assert (got["free"] == 128).all()
        pairs = [tuple(int(v) for v in row) for row in got["bound"]]
        for d, counts in want.items():
            assert all(pairs[i] == counts for i in np.flatnonzero(printed == d)) and (printed == d).any()
        if tag == "cc":       # the counts change exactly where the printed thousandths enter 3.004
            sweep = pairs[:41]
            assert {p for p, d in zip(sweep, printed[:41]) if d < 3004} == {(95, 95)}
            assert {p for p, d in zip(sweep, printed[:41]) if d >= 3004} == {(95, 96)}


# ---- 2. exclusions and radii ------------------------------------------------------------------------------------

def test_hydrogens_and_beads_cover_nothing_and_unknown_elements_take_1800(pkg, tmp_path):
    pkg.init(0)
    # a hydrogen of the receptor and a bead of the ligand halfway between two carbons 3 A apart
    rec, lig = pair_of_files(tmp_path, atom(1, "C", "GLY", "A", 1, (0, 0, 0), "C") + atom(2, "H", "GLY", "A", 1, (1.5, 0, 0), "H") +
                             atom(3, "D1", "GLY", "A", 1, (1.2, 0.5, 0), "D"),
                             atom(1, "BJ", "MMB", "B", 1, (-1.5, 0, 0), "C", True) + atom(2, "C", "GLY", "B", 2, (0, 0, 0), "C"))
    cx, rs = pkg.Complex(rec, lig), sr.SasaRestated(rec, lig)
    assert list(cx.sasa_radii(0)) == [1700, 0, 0] and list(cx.sasa_radii(1)) == [0, 1700]
    poses = rigid(1, [3.0])
    got = cx.sasa(poses, atoms=True)
    assert_equal(got, rs, poses)
    assert list(got["free"][0]) == [128, 0, 0, 0, 128] and list(got["bound"][0]) == [95, 0, 0, 0, 95]
    E2 = 3100 ** 2
    assert list(got["sums"][0]) == [128 * E2, 95 * E2, 128 * E2, 95 * E2]
    # radii by element, by atom name, of short records
    short = "ATOM      7  N   GLY A   3    %8.3f%8.3f%8.3f\n" % (40.0, 0.0, 0.0)
    assert len(short) == 55
    text = (atom(1, "ZN", "ZN", "A", 1, (0, 0, 0), "ZN", True) + atom(2, "X1", "UNK", "A", 2, (10, 0, 0), "") +
            atom(3, "CA", "GLY", "A", 3, (20, 0, 0), "") + atom(4, "SE", "MSE", "A", 4, (30, 0, 0), "se") + short +
            atom(8, "1HB", "ALA", "A", 5, (50, 0, 0), "") + atom(9, "CL", "CL", "A", 6, (60, 0, 0), "Cl", True) +
            atom(10, "O", "HOH", "A", 7, (70, 0, 0), " O") + atom(11, "BR", "UNK", "A", 8, (80, 0, 0), "BR") +
            atom(12, "I", "IOD", "A", 9, (90, 0, 0), " I") + atom(13, "F", "UNK", "A", 10, (100, 0, 0), " F") +
            atom(14, "P", "DA", "A", 11, (110, 0, 0), " P") + atom(15, "SG", "CYS", "A", 12, (120, 0, 0), " S"))
    rec, lig = pair_of_files(tmp_path, text, atom(1, "C", "GLY", "B", 1, (0, 0, 5.0), "C"), "radii")
    cx, rs = pkg.Complex(rec, lig), sr.SasaRestated(rec, lig)
    want = [1800, 1800, 1700, 1900, 1550, 0, 1750, 1520, 1850, 1980, 1470, 1800, 1800]
    assert list(cx.sasa_radii(0)) == want and list(rs.radii[:13]) == want
    assert np.array_equal(cx.sasa_radii(1), rs.radii[13:])
    poses = rigid(2, [0.0, 9.0])
    assert_equal(cx.sasa(poses, atoms=True), rs, poses)
    for name in ("1azp", "1k4c"):
        big, want = case_complex(pkg, name), sr.sasa_case(name)
        assert np.array_equal(np.concatenate([big.sasa_radii(0), big.sasa_radii(1)]), want.radii)
    with pytest.raises(pkg.LightdockError):
        cx.sasa_radii(2)
    d = pkg.sasa_directions()
    assert d.dtype == np.int32 and np.array_equal(d, sr.U)


# ---- 3. the golden complexes ------------------------------------------------------------------------------------

def test_1czy_ranked_models_and_final_glowworms(pkg, czy, czy_rs):
    entries = analyse_module().ranking(range(10), 100, base=CZY)
    assert len(entries) == 11
    poses = np.concatenate([np.array([e[2] for e in entries]), gso(2)[0][::25], gso(7)[0][3::25], gso(9)[0][5::25]])
    assert poses.shape == (11 + 24, 27)
    got = czy.sasa(poses, atoms=True)
    sums, _, _ = assert_equal(got, czy_rs, poses)
    assert [int(v) for v in got["sums"][0]] == [87964903100, 83835702000, 10636044500, 5434214900]
    buried = [round(sr.buried_area(s), 1) for s in sums[:11]]
    assert buried[0] == 916.1 and min(buried) == 408.6 and max(buried) == 916.1
    area = pkg.sasa_area(got["sums"][0])
    assert round(float(area[0] - area[1] + area[2] - area[3]), 1) == 916.1


def test_1azp_hydrogens_and_dna(pkg):
    cx, rs = case_complex(pkg, "1azp"), sr.sasa_case("1azp")
    poses = np.loadtxt(os.path.join(GOLDEN, "1azp", "initial_positions_0.dat"))[:8]
    assert poses.shape[1] == cx.pose_len == 27
    got = cx.sasa(poses, atoms=True)
    assert_equal(got, rs, poses)
    assert [int(v) for v in got["sums"][0]] == [48781775000, 45370010500, 33949188300, 29878156600]
    assert int((rs.radii[:1094] == 0).sum()) == 562 and int((rs.radii[1094:] == 0).sum()) == 178
    assert not got["free"][:, rs.radii == 0].any()


def test_1ppe_rigid_receptor_free_counts_do_not_move(pkg):
    cx, rs = case_complex(pkg, "1ppe"), sr.sasa_case("1ppe")
    rng = np.random.default_rng(11)
    poses = np.loadtxt(os.path.join(GOLDEN, "1ppe", "initial_positions_0.dat"))[:8, :7]
    poses[:, :3] += rng.normal(0, 1.5, (8, 3))
    got = cx.sasa(poses, atoms=True)
    assert_equal(got, rs, poses)
    n_rec = cx.num_atoms(0)
    assert (got["free"][:, :n_rec] == got["free"][0, :n_rec]).all() and (got["sums"][:, 0] == got["sums"][0, 0]).all()
    assert (got["free"][1:, n_rec:] != got["free"][0, n_rec:]).any()      # the directions stay, the ligand turns


def test_1k4c_membrane_complex(pkg):
    cx, rs = case_complex(pkg, "1k4c"), sr.sasa_case("1k4c")
    assert cx.num_atoms(0) + cx.num_atoms(1) == 6681 and int((rs.radii == 0).sum()) == 453
    poses = np.loadtxt(os.path.join(GOLDEN, "1k4c", "initial_positions_0.dat"))[:3, :7]
    got = cx.sasa(poses, atoms=True)
    assert_equal(got, rs, poses)
    assert [int(v) for v in got["sums"][0]] == [181471003400, 170728351300, 204947030800, 193178396100]


# ---- 4. far and out-of-range poses ------------------------------------------------------------------------------

def test_far_poses_bury_nothing_and_the_coordinate_bound(pkg, czy, czy_rs):
    base = gso(0)[0][:4].copy()
    far = base.copy()
    far[1, 0] += 500.0
    far[2, 1] = -0.9e6                       # inside the bound: a pose like any other
    got = czy.sasa(far, atoms=True)
    assert_equal(got, czy_rs, far)
    for i in (1, 2):
        assert np.array_equal(got["free"][i], got["bound"][i])
        s = [int(v) for v in got["sums"][i]]
        assert s[0] == s[1] and s[2] == s[3] and sr.buried_area(s) == 0.0
    assert not np.array_equal(got["free"][0], got["bound"][0])
    out = base.copy()
    out[3, 0] = 1.1e6
    with pytest.raises(pkg.LightdockError) as e:
        czy.sasa(out)
    assert e.value.status == -1


# ---- 5. a dense clump -------------------------------------------------------------------------------------------

def ball(rng, n, radius):
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    return v * radius * rng.uniform(0, 1, (n, 1)) ** (1.0 / 3.0)


def test_a_dense_clump_whose_lists_exceed_every_capacity(pkg, tmp_path):
    """700 receptor and 300 ligand atoms uniform in a ball of 4 A: every atom is every atom's neighbour, so every
    neighbour list is longer than the 128 entries a wave keeps."""
    rng = np.random.default_rng(2026)
    elements = ["C", "N", "O", "S"]
    rec = "".join(atom(i + 1, elements[i % 4], "UNK", "A", i + 1, xyz, elements[i % 4]) for i, xyz in enumerate(ball(rng, 700, 4.0)))
    lig = "".join(atom(i + 1, elements[i % 3], "UNK", "B", i + 1, xyz, elements[i % 3]) for i, xyz in enumerate(ball(rng, 300, 4.0)))
    rec, lig = pair_of_files(tmp_path, rec, lig)
    pkg.init(0)
    cx, rs = pkg.Complex(rec, lig), sr.SasaRestated(rec, lig)
    poses = rigid(2, [0.0, 2.5])
    got = cx.sasa(poses, atoms=True)
    assert_equal(got, rs, poses)
    assert (got["free"] == 0).mean() > 0.5 and (got["bound"] > 0).any() and (got["free"] > got["bound"]).any()


# ---- 6. a coarsened grid ----------------------------------------------------------------------------------------

def test_extents_that_coarsen_the_grid(pkg, tmp_path):
    """1k4c's receptor twice, 300 A apart: more than 4096 cells of 2 E_max, so the cells grow.  And two atoms 5000 A apart."""
    from conftest import case_paths
    _, d, rec, lig = case_paths("1k4c")
    lines = [l for l in open(rec) if l.startswith(("ATOM  ", "HETATM"))]
    far = [l[:21] + chr(ord(l[21]) + 10) + l[22:30] + "%8.3f" % (float(l[30:38]) + 300.0) + l[38:] for l in lines]
    twice = tmp_path / "twice.pdb"
    twice.write_text("".join(lines + far))
    pkg.init(0)
    cx, rs = pkg.Complex(str(twice), lig), sr.SasaRestated(str(twice), lig)
    poses = np.loadtxt(os.path.join(d, "initial_positions_0.dat"))[:2, :7]
    poses[1, 0] += 300.0                        # one pose at the copy
    got = cx.sasa(poses, atoms=True)
    assert_equal(got, rs, poses)
    n = 3413
    assert np.array_equal(got["free"][0, :n], got["free"][0, n:2 * n])      # the copy is the same molecule part, moved whole thousandths
    assert not np.array_equal(got["bound"][0, :n], got["bound"][0, n:2 * n])

    rec2, lig2 = pair_of_files(tmp_path, atom(1, "C", "GLY", "A", 1, (0, 0, 0), "C") + atom(2, "C", "GLY", "A", 2, (5000.0, 0, 0), "C"),
                               atom(1, "C", "GLY", "B", 1, (0, 0, 0), "C"), "two")
    cx, rs = pkg.Complex(rec2, lig2), sr.SasaRestated(rec2, lig2)
    poses = rigid(3, [3.0, 5003.0, 2500.0])
    got = cx.sasa(poses, atoms=True)
    assert_equal(got, rs, poses)
    assert [list(r) for r in got["bound"]] == [[95, 128, 95], [128, 95, 95], [128, 128, 128]]


# ---- 7. batch invariance and slot reuse -------------------------------------------------------------------------

def raw_call(lib, cx, poses, probe=1.4, want=(True, True, True), stride=None, n_atoms=None):
    """ld_complex_sasa on buffers filled with 0xA5 -> (status, sums, free, bound) (None where not asked for)."""
    poses = np.ascontiguousarray(poses, dtype=np.float64)
    n = len(poses)
    n_atoms = cx.num_atoms(0) + cx.num_atoms(1) if n_atoms is None else n_atoms
    bufs = [np.full((n, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64), np.full((n, n_atoms), FILL, dtype=np.uint8),
            np.full((n, n_atoms), FILL, dtype=np.uint8)]
    bufs = [b if w else None for b, w in zip(bufs, want)]
    ptrs = [None if b is None else b.ctypes.data_as(ctypes.c_void_p) for b in bufs]
    status = lib.ld_complex_sasa(cx._h, n, poses.ctypes.data_as(ctypes.c_void_p), poses.shape[1] if stride is None else stride,
                                 ctypes.c_double(probe), *ptrs)
    return (status,) + tuple(bufs)


def untouched(bufs):
    return all(b is None or (b.view(np.uint8) == FILL).all() for b in bufs)


def test_3000_poses_in_one_call_and_in_pieces(pkg, czy, czy_rs):
    poses = perturbed_czy(np.random.default_rng(5), 15).reshape(3000, 27)
    whole = czy.sasa(poses, atoms=True)           # more poses than the 1024 slots: every slot is reused
    print("3000 1czy poses: sasa kernel %.3f ms" % czy.last_kernel_ms())
    cuts = (0, 701, 1790, 3000)
    pieces = [czy.sasa(poses[a:b], atoms=True) for a, b in zip(cuts, cuts[1:])]
    for key in ("sums", "free", "bound"):
        assert np.concatenate([p[key] for p in pieces]).tobytes() == whole[key].tobytes()
    assert np.array_equal(czy.sasa(poses)["sums"], whole["sums"])
    rows = [0, 1023, 1024, 1999, 2048, 2999]
    sums, free, bound = czy_rs.batch(poses[rows])
    assert np.array_equal(whole["sums"][rows], sums) and np.array_equal(whole["free"][rows], free)
    assert np.array_equal(whole["bound"][rows], bound)
    lib = pkg.load_library()
    for want in itertools.product((False, True), repeat=3):
        status, s, f, b = raw_call(lib, czy, poses[:5], want=want)
        assert status == 0
        assert s is None or np.array_equal(s, whole["sums"][:5])
        assert f is None or np.array_equal(f, whole["free"][:5])
        assert b is None or np.array_equal(b, whole["bound"][:5])
    empty = czy.sasa(np.zeros((0, 27)), atoms=True)
    assert empty["sums"].shape == (0, 4) and empty["free"].shape == (0, czy.num_atoms(0) + czy.num_atoms(1))
    assert lib.ld_complex_sasa(czy._h, 0, None, 27, ctypes.c_double(1.4), None, None, None) == 0


# ---- 8. probes and refusals -------------------------------------------------------------------------------------

def test_probes_and_refusals(pkg, czy, czy_rs, tmp_path):
    poses = np.stack([gso(0)[0][0], gso(5)[0][100], gso(9)[0][199]])
    for probe in (0.0, 1.4, 2.0):
        assert_equal(czy.sasa(poses, probe, atoms=True), czy_rs, poses, probe)
    lib = pkg.load_library()

    def refused(p, probe=1.4, stride=None, cx=czy):
        out = raw_call(lib, cx, p, probe, stride=stride)
        assert out[0] == -1 and lib.ld_last_error().decode()
        assert untouched(out[1:])

    for probe in (-0.001, -1.0, 2.001, float("nan"), float("inf"), -float("inf"), 1e300):
        refused(poses, probe)
        with pytest.raises(pkg.LightdockError):
            czy.sasa(poses, probe)
    for bad in (np.nan, np.inf, -np.inf):
        p = poses.copy()
        p[1, 5] = bad
        refused(p)
    z = poses.copy()
    z[2, 3:7] = 0.0
    refused(z)
    refused(poses[:, :20])                    # stride below the pose length
    over = poses.copy()
    over[2, 2] = -1.1e6                       # beyond the coordinate bound, found by the kernel
    refused(over)
    ok = raw_call(lib, czy, poses)
    assert ok[0] == 0 and not untouched(ok[1:])
    # a side of which no atom takes part
    rec, lig = pair_of_files(tmp_path, atom(1, "C", "GLY", "A", 1, (0, 0, 0), "C"),
                             atom(1, "H", "GLY", "B", 1, (0, 0, 0), "H") + atom(2, "BJ", "MMB", "B", 2, (1, 0, 0), "C", True))
    for a, b in ((rec, lig), (lig, rec)):
        cx = pkg.Complex(a, b)
        refused(rigid(2, [0.0, 3.0]), cx=cx)
        assert sorted(list(cx.sasa_radii(0)) + list(cx.sasa_radii(1))) == [0, 0, 1700]


# ---- 9. the PDB tie ---------------------------------------------------------------------------------------------

def test_the_surface_of_a_pose_is_that_of_the_pdb_file_written_for_it(czy, czy_rs, tmp_path):
    poses = np.stack([gso(0)[0][0], gso(3)[0][17], gso(9)[0][199]])
    got = czy.sasa(poses, atoms=True)
    for i, p in enumerate(poses):
        path = str(tmp_path / ("m%d.pdb" % i))
        czy.write_pdb(p, path)
        xyz, _ = read_pdb(path)                      # the numbers of the file's text
        free, bound, sums = czy_rs.of_xyz(xyz)
        assert np.array_equal(got["free"][i], free) and np.array_equal(got["bound"][i], bound)
        assert [int(v) for v in got["sums"][i]] == sums


# ---- 10. interface.py end to end --------------------------------------------------------------------------------

def run_interface(pkg, run, *args):
    script = os.path.join(os.path.dirname(pkg.__file__), "interface.py")
    r = subprocess.run([sys.executable, script] + list(args), cwd=run, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout, open(os.path.join(run, "interface", "buried_area.list")).read().splitlines()


def test_interface_tool_on_a_copy_of_the_1czy_run(pkg, czy, czy_rs, tmp_path):
    tool = tool_module("interface")
    entries = analyse_module().ranking(range(10), 100, base=CZY)
    run = tmp_path / "run"
    shutil.copytree(CZY, run)
    out, lines = run_interface(pkg, run, "setup.json", "100", "--swarms", "0-9", "--top", "2")
    assert "11 models measured" in out and len(lines) == 12
    restated = [czy_rs.sasa(e[2]) for e in entries]
    want = []
    for e, (_, _, s) in zip(entries, restated):
        rec, lig, both = s[0] * sr.AREA, s[2] * sr.AREA, (s[1] + s[3]) * sr.AREA
        want.append("%5d %9d %11.5f %9.1f %9.1f %9.1f %9.1f" % (e[0], e[1], e[3]["scoring"], rec, lig, both, sr.buried_area(s)))
    assert lines[1:] == want
    buried = [float(l.split()[6]) for l in lines[1:]]
    assert buried[0] == 916.1 and min(buried) == 408.6 and max(buried) == 916.1
    assert sorted(os.listdir(run / "interface")) == ["buried_area.list", "residues_1.list", "residues_2.list"]
    n_rec = len(czy_rs.rec)
    for k in (0, 1):
        free, bound, _ = restated[k]
        rows = []
        for tag, ids, of, cut in (("R", czy_rs.rec_ids, czy_rs.rec_of, slice(0, n_rec)), ("L", czy_rs.lig_ids, czy_rs.lig_of, slice(n_rec, None))):
            f, b = sr.residue_areas(free[cut], bound[cut], czy_rs.radii[cut], of)
            rows += [[tag, ids[r], "%.1f" % (int(f[r]) * sr.AREA), "%.1f" % (int(b[r]) * sr.AREA), "%.1f" % ((int(f[r]) - int(b[r])) * sr.AREA)]
                     for r in np.flatnonzero(f > b)]
        header, got = tool.parse_list(open(run / "interface" / ("residues_%d.list" % (k + 1))).read())
        assert header == ["Side", "Residue", "Free", "Bound", "Buried"] and got == rows and len(rows) > 5
    out, lines = run_interface(pkg, run, "setup.json", "100", "--all", "--swarms", "0")
    assert "200 models measured" in out and len(lines) == 201
    scores = [float(l.split()[2]) for l in lines[1:]]
    assert scores == sorted(scores, reverse=True)


# ---- 11. time ---------------------------------------------------------------------------------------------------

def test_sasa_of_1024_1k4c_poses_is_far_below_all_pairs(pkg):
    """1024 jittered 1k4c poses, HIP events, median of 5 after a warm-up.  The gate is derived from the atom counts: all
    points against all atoms is N x 128 x (N - 1) tests a pose (N atoms take part), at 7 vector instructions a test on 64
    lanes, 2 cycles an instruction, 2.4 GHz and 1024 SIMDs: 0.44 ms of pure issue a pose for 1k4c.  A neighbour-limited
    kernel does about a hundredth of those tests; the gate is a quarter of the all-pairs figure.
    Measured 2026-10-19 on one MI355X: T_sasa 21.2 ms, T_contacts 0.23 ms, all pairs 452.5 ms, gate 113.1 ms."""
    from conftest import case_paths
    _, d, rec, lig = case_paths("1k4c")
    pkg.init(0)
    base = np.loadtxt(os.path.join(d, "initial_positions_0.dat"))[:, :7]
    poses = pkg.synth.jitter(base, 1024, seed=17)
    cx = pkg.Complex(rec, lig)
    N = int((cx.sasa_radii(0) > 0).sum() + (cx.sasa_radii(1) > 0).sum())
    assert N == 6681 - 453
    all_pairs_ms = N * 128.0 * (N - 1) / 64.0 * 7 * 2 / 2.4e9 / 1024 * 1e3
    assert 0.43 < all_pairs_ms < 0.45
    first = cx.sasa(poses)                                    # warm-up
    times = []
    for _ in range(5):
        again = cx.sasa(poses)
        times.append(cx.last_kernel_ms())
    t_sasa = float(np.median(times))
    assert np.array_equal(first["sums"], again["sums"])
    rs = sr.sasa_case("1k4c")
    assert [int(v) for v in first["sums"][1023]] == rs.sasa(poses[1023])[2]
    cx.contacts(poses, packed=True)
    times = []
    for _ in range(5):
        cx.contacts(poses, packed=True)
        times.append(cx.last_kernel_ms())
    t_contacts = float(np.median(times))
    gate = 0.25 * all_pairs_ms * 1024
    print("1024 1k4c poses: T_sasa %.3f ms, T_contacts %.3f ms, all pairs %.1f ms, gate %.1f ms" % (t_sasa, t_contacts, all_pairs_ms * 1024, gate))
    assert t_sasa <= gate
