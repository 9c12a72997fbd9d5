"""Model quality against a reference complex (ld_complex_assess, lightdock-rust_amd/assess.py) on the CPU:
a restatement of the rule in include/lightdock_hip.h ("Model quality") that the GPU tests import -- matching and native
pairs by the column rule in numpy int64, the sums as Python integers, the largest eigenvalue as the largest root of the exact
characteristic quartic (Newton in `decimal` at 60 digits), a numpy SVD Kabsch for L-RMSD -- tested on constructions whose
answer is known, pinned on the counts of the fixtures, and assess.py's arithmetic and text."""
import decimal
import functools
import os

import numpy as np
import pytest

from test_analysis_cpu import CZY, ROOT, analyse_module, restated_pdb, tool_module
from test_contacts_cpu import GOLDEN, ContactsRestated, atom_contacts, thousandths

FIT_NAMES = ("N", "CA", "C", "O", "P")
EPS = 2.0 ** -52


def assess_module():
    return tool_module("assess")


# ---- the restatement --------------------------------------------------------------------------------------------

def records(path):
    return [l.rstrip("\r\n") for l in open(path) if l.startswith(("ATOM  ", "HETATM"))]


def record_key(line):
    """chain (column 22), sequence number (23-26), insertion code (27), residue name (18-20), atom name (13-16)."""
    return tuple(f.strip(" ") for f in (line[21], line[22:26], line[26], line[17:20], line[12:16]))


def match(model_lines, ref_lines):
    """For every model record the index of the FIRST reference record with the same key, -1 without one."""
    first = {}
    for i, l in enumerate(ref_lines):
        first.setdefault(record_key(l), i)
    return np.array([first.get(record_key(l), -1) for l in model_lines], dtype=np.int64)


def fast_thousandths(xyz):
    """test_contacts_cpu.thousandths, vectorised: rint(x * 1000) wherever the product is not within 1e-6 of a tie (there its
    rounding error, below 1e-9, cannot change the result), the printed text elsewhere."""
    x = np.asarray(xyz, dtype=np.float64)
    p = x * 1000.0
    out = np.rint(p).astype(np.int64)
    tie = np.abs(p - np.floor(p) - 0.5) < 1e-6
    if tie.any():
        out[tie] = thousandths(x[tie])
    return out


def det3(m):
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
            m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


def det4(m):
    return sum((-1) ** j * m[0][j] * det3([[row[k] for k in range(4) if k != j] for row in m[1:]]) for j in range(4))


def exact_sums(m, r):
    """m, r: int64 (n, 3) thousandths -> Python integers n, A = n sum|m - mean|^2, B likewise of r, K = n sum (m - mean)(r - mean)^T."""
    n = len(m)
    M = [[int(v) for v in row] for row in m]
    R = [[int(v) for v in row] for row in r]
    sm = [sum(p[a] for p in M) for a in range(3)]
    sr = [sum(p[a] for p in R) for a in range(3)]
    A = n * sum(v * v for p in M for v in p) - sum(v * v for v in sm)
    B = n * sum(v * v for p in R for v in p) - sum(v * v for v in sr)
    K = [[n * sum(p[a] * q[b] for p, q in zip(M, R)) - sm[a] * sr[b] for b in range(3)] for a in range(3)]
    return n, A, B, K


def exact_fit(m, r):
    """The best proper superposition of m on r, exactly: (rmsd^2 in A^2, G_m, G_r in A^2).  n lambda is the largest root of
    the characteristic quartic x^4 + c2 x^2 + c1 x + c0 of Horn's matrix of K (trace 0), by Newton from the upper bound
    (A + B) / 2, beyond which the quartic is convex and increasing."""
    n, A, B, K = exact_sums(m, r)
    (xx, xy, xz), (yx, yy, yz), (zx, zy, zz) = K
    N = [[xx + yy + zz, yz - zy, zx - xz, xy - yx], [yz - zy, xx - yy - zz, xy + yx, zx + xz],
         [zx - xz, xy + yx, -xx + yy - zz, yz + zy], [xy - yx, zx + xz, yz + zy, -xx - yy + zz]]
    D = decimal.Decimal
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        c2, c1, c0 = D(-2 * sum(v * v for row in K for v in row)), D(-8 * det3(K)), D(det4(N))
        x = D(A + B) / 2
        for _ in range(1000):
            f, df = ((x * x + c2) * x + c1) * x + c0, (4 * x * x + 2 * c2) * x + c1
            if df == 0:
                break
            step = f / df
            x -= step
            if abs(step) <= abs(x) * D(10) ** -45:
                break
        rmsd2 = max(D(0), (D(A + B) - 2 * x) / D(n * n)) / D(10 ** 6)
        return float(rmsd2), float(D(A) / D(n) / D(10 ** 6)), float(D(B) / D(n) / D(10 ** 6))


def kabsch(P, Q):
    """The proper rotation R (numpy SVD, determinant corrected) with R p ~ q for centred P, Q (n, 3)."""
    U, _, Vt = np.linalg.svd(P.T @ Q)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    return Vt.T @ np.diag([1.0, 1.0, d]) @ U.T


def svd_lrmsd(m_rec, r_rec, m_lig, r_lig):
    """int64 thousandths -> (L-RMSD^2 in A^2, G_l,m, G_l,r in A^2 about the receptor's fit centroids)."""
    cm, cr = np.rint(m_rec.mean(axis=0)).astype(np.int64), np.rint(r_rec.mean(axis=0)).astype(np.int64)   # exact shifts first
    P, Q, PL, QL = ((a - c) / 1000.0 for a, c in ((m_rec, cm), (r_rec, cr), (m_lig, cm), (r_lig, cr)))
    pm, qm = P.mean(axis=0), Q.mean(axis=0)
    R = kabsch(P - pm, Q - qm)
    PL, QL = PL - pm, QL - qm
    d = PL @ R.T - QL
    return float((d * d).sum() / len(PL)), float((PL * PL).sum()), float((QL * QL).sum())


class AssessRestated(ContactsRestated):
    """The rule of lightdock_hip.h, "Model quality", restated."""

    def __init__(self, rec_pdb, lig_pdb, rec_modes, lig_modes, ref_rec, ref_lig, contact_cutoff=5.0, interface_cutoff=10.0):
        ContactsRestated.__init__(self, rec_pdb, lig_pdb, rec_modes, lig_modes)
        self.cutoff = contact_cutoff
        lines = records(rec_pdb) + records(lig_pdb)
        n_rec = self.n_rec = len(self.rec)
        of = np.concatenate([match(records(rec_pdb), records(ref_rec)), match(records(lig_pdb), records(ref_lig))])
        ref_xyz = np.array([[float(l[30:38]), float(l[38:46]), float(l[46:54])] for l in records(ref_rec) + records(ref_lig)])
        n_ref_rec = len(records(ref_rec))
        self.matched = of >= 0
        src = np.where(np.arange(len(of)) < n_rec, of, of + n_ref_rec)
        self.ref_t = np.zeros((len(of), 3), dtype=np.int64)
        self.ref_t[self.matched] = np.rint(ref_xyz[src[self.matched]] * 1000.0).astype(np.int64)      # llrint(x * 1000)
        self.fit = self.matched & np.array([l[12:16].strip(" ") in FIT_NAMES for l in lines])
        self.res = np.concatenate([self.rec_of, self.lig_of + len(self.rec_ids)])        # residue of every complex atom
        side = np.arange(len(of)) >= n_rec
        ra, la = np.flatnonzero(self.matched & ~side), np.flatnonzero(self.matched & side)
        near = atom_contacts(self.ref_t[ra], self.ref_t[la], contact_cutoff)
        i, j = np.nonzero(near)
        self.native = sorted(set(zip(self.res[ra][i].tolist(), (self.res[la][j] - len(self.rec_ids)).tolist())))
        wide = atom_contacts(self.ref_t[ra], self.ref_t[la], interface_cutoff)
        interface = np.zeros(len(self.rec_ids) + len(self.lig_ids), dtype=bool)
        interface[self.res[ra][wide.any(axis=1)]] = True
        interface[self.res[la][wide.any(axis=0)]] = True
        self.interface_fit = self.fit & interface[self.res]
        in_native = np.zeros(len(interface), dtype=bool)
        for a, b in self.native:
            in_native[a] = in_native[b + len(self.rec_ids)] = True
        self.used = self.matched & (self.fit | in_native[self.res])
        self.pair_atoms = [(np.flatnonzero(self.matched & (self.res == a)), np.flatnonzero(self.matched & (self.res == b + len(self.rec_ids))))
                           for a, b in self.native]
        self.rec_fit, self.lig_fit = self.fit & ~side, self.fit & side

    def counts(self):
        return {"matched_rec": int(self.matched[:self.n_rec].sum()), "matched_lig": int(self.matched[self.n_rec:].sum()),
                "native_pairs": len(self.native), "rec_fit": int(self.rec_fit.sum()), "lig_fit": int(self.lig_fit.sum()),
                "interface_fit": int(self.interface_fit.sum())}

    def posed_thousandths(self, row, ligand_frame=True):
        t = np.zeros((len(self.used), 3), dtype=np.int64)
        t[self.used] = fast_thousandths(self.pose(row, ligand_frame)[self.used])
        return t

    def measures_of(self, t):
        """Complex thousandths (used atoms at least) -> dict: kept, irmsd2 (exact), its G_a, G_b, lrmsd2 (SVD), its G_la, G_lb."""
        kept = sum(bool(atom_contacts(t[a], t[b], self.cutoff).any()) for a, b in self.pair_atoms)
        i2, ga, gb = exact_fit(t[self.interface_fit], self.ref_t[self.interface_fit])
        l2, gla, glb = svd_lrmsd(t[self.rec_fit], self.ref_t[self.rec_fit], t[self.lig_fit], self.ref_t[self.lig_fit])
        return {"kept": kept, "irmsd2": i2, "ga": ga, "gb": gb, "lrmsd2": l2, "gla": gla, "glb": glb}

    def measures(self, row, ligand_frame=True):
        return self.measures_of(self.posed_thousandths(row, ligand_frame))

    def bounds(self, m):
        """The tolerances of the GPU tests on irmsd^2 and lrmsd^2 for the measures m of one pose."""
        return 64 * EPS * (m["ga"] + m["gb"]) / int(self.interface_fit.sum()), 128 * EPS * (m["gla"] + m["glb"]) / int(self.lig_fit.sum())


# ---- reference files for the tests ------------------------------------------------------------------------------

FRAME_Q = np.array([0.3, -0.5, 0.7, 0.4]) / np.linalg.norm([0.3, -0.5, 0.7, 0.4])
FRAME_T = np.array([12.345, -67.8, 30.1])


def quaternion_matrix(q):
    w, x, y, z = q
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def moved(lines, R, t):
    """Records in another frame, reprinted with %8.3f."""
    out = []
    for l in lines:
        x = R @ np.array([float(l[30:38]), float(l[38:46]), float(l[46:54])]) + t
        out.append(l[:30] + "%8.3f%8.3f%8.3f" % tuple(x) + l[54:])
    return out


def disturbed(lines):
    """A handful of records deleted, one residue renamed, two records swapped, and a duplicate of a record (elsewhere in space)
    appended: matching by key, the first record wins."""
    lines = list(lines)
    third = [i for i, l in enumerate(lines) if l[17:27] == lines[len(lines) // 3][17:27]]
    for i in third:
        lines[i] = lines[i][:17] + "UNK" + lines[i][20:]
    lines[10], lines[11] = lines[11], lines[10]
    dup = lines[2][:30] + "%8.3f%8.3f%8.3f" % (99.0, 99.0, 99.0) + lines[2][54:]
    for i in sorted({1, 7, len(lines) // 2, len(lines) - 2}, reverse=True):
        del lines[i]
    return lines + [dup]


def write_reference(model_text, n_rec, directory, name, frame=True, disturb=True):
    """model_text: the PDB text of a posed model (ld_complex_write_pdb's, or test_analysis_cpu.restated_pdb's) -> the paths of a
    reference receptor and ligand made of it."""
    lines = model_text.splitlines()
    parts = [lines[:n_rec], lines[n_rec:]]
    if frame:
        R = quaternion_matrix(FRAME_Q)
        parts = [moved(p, R, FRAME_T) for p in parts]
    if disturb:
        parts = [disturbed(p) for p in parts]
    paths = []
    for side, p in zip(("rec", "lig"), parts):
        paths.append(os.path.join(str(directory), "%s_%s.pdb" % (name, side)))
        with open(paths[-1], "w") as f:
            f.write("".join(l + "\n" for l in p))
    return paths


def case_files(name):
    """(receptor pdb, ligand pdb, receptor modes, ligand modes) of a golden case; 1czy from its run directory."""
    if name == "1czy":
        return (os.path.join(CZY, "lightdock_1czy_protein.pdb"), os.path.join(CZY, "lightdock_1czy_peptide.pdb"),
                np.load(os.path.join(CZY, "lightdock_rec.nm.npy")), np.load(os.path.join(CZY, "lightdock_lig.nm.npy")))
    from conftest import case_paths
    c, d, rec, lig = case_paths(name)
    if c["use_anm"]:
        return rec, lig, np.load(os.path.join(d, "rec_nm.npy")), np.load(os.path.join(d, "lig_nm.npy"))
    return rec, lig, None, None


def case_poses(name):
    """The poses of a fixture and the index of the one its reference is made of."""
    an = analyse_module()
    if name == "1czy":
        return np.concatenate([an.read_gso(os.path.join(CZY, "swarm_%d" % s, "gso_100.out"))[0] for s in range(10)]), 2 * 200 + 74
    if name == "1azp":
        return an.read_gso(os.path.join(GOLDEN, "1azp", "swarm_0", "gso_100.out"))[0], REFERENCE_POSE[name]
    rows = np.loadtxt(os.path.join(GOLDEN, name, "initial_positions_0.dat"))
    n, width = {"1ppe": (120, 7), "1k4c": (32, 7), "ab_icode": (48, rows.shape[1])}[name]
    return rows[:n, :width], REFERENCE_POSE[name]


REFERENCE_POSE = {"1azp": 0, "1ppe": 0, "1k4c": 0, "ab_icode": 0}


@functools.lru_cache(maxsize=None)
def restated_case(name, directory, frame=True, disturb=True):
    """The fixture `name` with a reference made from the restatement's own text of its reference pose (what
    ld_complex_write_pdb writes, byte for byte: tests/test_gpu_analysis.py) -> (AssessRestated, reference paths, poses)."""
    rec, lig, rm, lm = case_files(name)
    poses, k = case_poses(name)
    plain = ContactsRestated(rec, lig, rm, lm)
    paths = write_reference(restated_pdb(plain, rec, lig, poses[k]), len(plain.rec), directory, "%s_%d%d" % (name, frame, disturb), frame, disturb)
    return AssessRestated(rec, lig, rm, lm, paths[0], paths[1]), paths, poses


# ---- the restatement on constructions whose answer is known ------------------------------------------------------

CHIRAL = np.array([[0, 0, 0], [1500, 0, 0], [0, 2500, 0], [300, 400, 3500]], dtype=np.int64)


def test_identical_sets_and_half_turns_fit_exactly():
    assert exact_fit(CHIRAL, CHIRAL)[0] == 0.0
    for axis in range(3):
        s = -np.ones(3, dtype=np.int64)
        s[axis] = 1
        turned = CHIRAL * s + np.array([1999000, -1999000, 7])
        rmsd2, ga, gb = exact_fit(turned, CHIRAL)
        assert rmsd2 < 1e-40 and ga == gb > 0
        l2, _, _ = svd_lrmsd(turned, CHIRAL, turned[:2], CHIRAL[:2])
        assert l2 < 1e-12


def test_a_mirror_image_is_not_a_fit():
    mirror = CHIRAL * np.array([1, 1, -1])
    rmsd2, _, _ = exact_fit(mirror, CHIRAL)
    assert rmsd2 > 0.01
    # the SVD without the determinant correction would call it a fit; with it, it agrees with the quartic
    P, Q = (a - a.mean(axis=0) for a in (mirror / 1000.0, CHIRAL / 1000.0))
    d = P @ kabsch(P, Q).T - Q
    assert abs((d * d).sum() / 4 - rmsd2) < 1e-12
    assert np.linalg.det(kabsch(P, Q)) > 0


def test_a_known_misfit():
    turned = np.stack([-CHIRAL[:, 1], CHIRAL[:, 0], CHIRAL[:, 2]], axis=1)           # a quarter turn about z
    lig_ref = np.array([[9000, 0, 0], [9000, 1000, 0]], dtype=np.int64)
    lig_model = np.array([[0, 9000, 0], [-1000, 9000, 1000]], dtype=np.int64)        # turned; the second atom 1 A up
    l2, _, _ = svd_lrmsd(turned, CHIRAL, lig_model, lig_ref)
    assert abs(l2 - 0.5) < 1e-12
    lifted = turned.copy()
    lifted[3, 2] += 1000
    assert 0.0 < exact_fit(lifted, CHIRAL)[0] < 0.25                                 # below the unfitted 1 A^2 / 4


def pdb_line(serial, name, resname, chain, seq, xyz, icode=" "):
    return "ATOM  %5d %-4s %3s %1s%4d%1s   %8.3f%8.3f%8.3f  1.00  0.00\n" % ((serial, name, resname, chain, seq, icode) + tuple(xyz))


def tiny_complex(directory, lig_at=(3.0, 4.0, 0.0)):
    """Receptor: N, CA, C and a CB of one glycine; ligand: one P, 3-4-5 from the N, and an OP1 far away."""
    rec, lig = os.path.join(str(directory), "rec.pdb"), os.path.join(str(directory), "lig.pdb")
    with open(rec, "w") as f:
        f.write(pdb_line(1, " N", "GLY", "A", 1, (0, 0, 0)) + pdb_line(2, " CA", "GLY", "A", 1, (-1.5, 0, 0)) +
                pdb_line(3, " C", "GLY", "A", 1, (1.5, 1.5, 20)) + pdb_line(4, " CB", "GLY", "A", 1, (0, 1.5, 20)))
    with open(lig, "w") as f:
        f.write(pdb_line(1, " P", " DT", "B", 1, lig_at) + pdb_line(2, " OP1", " DT", "B", 1, (30.0, 30.0, 30.0)))
    return rec, lig


def test_native_pair_at_exactly_the_cutoff(tmp_path):
    rec, lig = tiny_complex(tmp_path)
    rs = AssessRestated(rec, lig, None, None, rec, lig, 5.0, 10.0)                   # 3-4-5: 25 000 000 <= 5000^2
    assert rs.native == [(0, 0)] and rs.counts() == {"matched_rec": 4, "matched_lig": 2, "native_pairs": 1, "rec_fit": 3,
                                                     "lig_fit": 1, "interface_fit": 4}
    assert AssessRestated(rec, lig, None, None, rec, lig, 4.999, 10.0).native == []
    still = np.array([0, 0, 0, 1, 0, 0, 0.0])
    m = rs.measures(still)
    assert m["kept"] == 1 and m["irmsd2"] == 0.0 and m["lrmsd2"] < 1e-20
    step = still.copy()
    step[0] = 0.001                                                                  # the P one thousandth further: 3.001-4-5
    assert rs.measures(step)["kept"] == 0


def test_matching_takes_the_first_record_and_trims_blanks(tmp_path):
    rec, lig = tiny_complex(tmp_path)
    ref = tmp_path / "ref_rec.pdb"
    lines = open(rec).read().splitlines()
    lines = [lines[1], lines[0], lines[3], lines[0][:30] + "%8.3f%8.3f%8.3f" % (50, 50, 50) + lines[0][54:]]   # C gone, N twice
    ref.write_text("".join(l + "\n" for l in lines))
    of = match(records(rec), records(str(ref)))
    assert list(of) == [1, 0, -1, 2]
    assert record_key(pdb_line(7, "CA", "GLY", "A", 12, (0, 0, 0), "B")) == ("A", "12", "B", "GLY", "CA")


def test_fast_thousandths_is_the_printed_number():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.uniform(-2000, 2000, 20000), np.arange(-50, 50) / 2000.0 + 1e-13, [0.0005, 2.0005, -0.0004, 4.9995, 123.4565]])
    assert np.array_equal(fast_thousandths(x), thousandths(x))


# ---- the fixtures, pinned ---------------------------------------------------------------------------------------

def test_reference_counts_of_the_fixtures(tmp_path):
    rs, paths, poses = restated_case("1czy", str(tmp_path))
    assert len(poses) == 2000
    assert rs.counts() == PINNED["1czy"]
    own = rs.measures(poses[474])
    assert own["kept"] == len(rs.native) and own["irmsd2"] < 1e-5 and own["lrmsd2"] < 1e-5     # printed twice: not 0
    plain, _, _ = restated_case("1czy", str(tmp_path), False, False)
    assert plain.counts() == PINNED["1czy plain"]
    own = plain.measures(poses[474])
    assert own["kept"] == len(plain.native) and own["irmsd2"] < 1e-20 and own["lrmsd2"] < 1e-20
    for name in ("1azp", "1ppe", "1k4c", "ab_icode"):
        rs, _, _ = restated_case(name, str(tmp_path))
        assert rs.counts() == PINNED[name]


def _counts(*v):
    return dict(zip(("matched_rec", "matched_lig", "native_pairs", "rec_fit", "lig_fit", "interface_fit"), v))


PINNED = {"1czy": _counts(1268, 40, 25, 665, 21, 245), "1czy plain": _counts(1281, 53, 31, 672, 28, 260),
          "1azp": _counts(1068, 472, 14, 258, 14, 91), "1ppe": _counts(1601, 208, 43, 874, 109, 285),
          "1k4c": _counts(3402, 3258, 313, 1562, 1707, 1059), "ab_icode": _counts(3314, 260, 72, 1742, 130, 298)}


# ---- assess.py's arithmetic and text ----------------------------------------------------------------------------

def test_dockq_and_the_capri_classes_at_each_boundary():
    am = assess_module()
    assert am.dockq(1.0, 0.0, 0.0) == 1.0
    assert abs(am.dockq(0.0, 1.5, 8.5) - (0.5 + 0.5) / 3.0) < 1e-15
    assert np.allclose(am.dockq([0.5, 0.2], [1.5, 3.0], [8.5, 17.0]), [(0.5 + 0.5 + 0.5) / 3, (0.2 + 0.2 + 0.2) / 3])
    c = am.capri_class
    assert c(0.5, 1.0, 99.0) == "high" and c(0.5, 99.0, 1.0) == "high"
    assert c(0.499, 1.0, 1.0) == "medium" and c(0.5, 1.001, 1.001) == "medium"
    assert c(0.3, 2.0, 99.0) == "medium" and c(0.3, 99.0, 5.0) == "medium"
    assert c(0.299, 2.0, 5.0) == "acceptable" and c(0.3, 2.001, 5.001) == "acceptable" and c(1.0, 2.001, 5.001) == "acceptable"
    assert c(0.1, 4.0, 99.0) == "acceptable" and c(0.1, 99.0, 10.0) == "acceptable"
    assert c(0.099, 0.0, 0.0) == "incorrect" and c(0.1, 4.001, 10.001) == "incorrect" and c(1.0, 4.001, 10.001) == "incorrect"


def test_the_text_of_assessment_list():
    am = assess_module()
    entries = [(2, 74, None, {"scoring": 19.37247}), (0, 3, None, {"scoring": -2.0}), (11, 199, None, {"scoring": 7.25})]
    fnat, irmsd, lrmsd = np.array([1.0, 0.0, 1 / 3.0]), np.array([0.0004, 12.3456, 1.9996]), np.array([0.0, 40.25, 4.5])
    assert am.assessment_text(entries, fnat, irmsd, lrmsd) == (
        "Swarm  Glowworm     Scoring    fnat    iRMSD    LRMSD   DockQ  CAPRI\n"
        "    2        74    19.37247   1.000    0.000    0.000   1.000  high\n"
        "    0         3    -2.00000   0.000   12.346   40.250   0.019  incorrect\n"
        "   11       199     7.25000   0.333    2.000    4.500   0.492  medium\n")
    assert am.assessment_text([], fnat[:0], irmsd[:0], lrmsd[:0]) == am.ASSESS_HEADER
