"""Interface contacts (ld_complex_contacts, lightdock-rust_amd/filter.py) on the CPU: an int64 numpy
restatement of the rule in include/lightdock_hip.h (the checker the GPU tests use), pinned on counts of the committed runs,
and filter.py's file logic on hand-made arrays."""
import os

import numpy as np
import pytest

from test_analysis_cpu import CZY, ROOT, Restated, analyse_module, tool_module

GOLDEN = os.path.join(ROOT, "tests", "golden")


def filter_module():
    return tool_module("filter")


# ---- the restatement --------------------------------------------------------------------------------------------

def read_residues(path):
    """Residues of a PDB file by the column rule: maximal runs of consecutive ATOM/HETATM records with the same chain
    (column 22), residue name (18-20), sequence number (23-26) and insertion code (27).
    -> (residue index of every atom, ids "<chain>.<resname>.<serial><icode>")."""
    of, ids, last = [], [], None
    for line in open(path):
        if line.startswith(("ATOM  ", "HETATM")):
            key = (line[21], line[17:20], line[22:26], line[26])
            if key != last:
                ids.append("%s.%s.%d%s" % (line[21].strip(), line[17:20].strip(), int(line[22:26]), line[26].strip()))
                last = key
            of.append(len(ids) - 1)
    return np.array(of), ids


def thousandths(xyz):
    """Every coordinate as the integer number of thousandths "%.3f" prints."""
    flat = [int(("%.3f" % v).replace(".", "")) for v in np.asarray(xyz, dtype=np.float64).ravel()]
    return np.array(flat, dtype=np.int64).reshape(np.shape(xyz))


def atom_contacts(rec_t, lig_t, cutoff):
    """bool (receptor atoms, ligand atoms): dx^2 + dy^2 + dz^2 <= C^2 on int64 thousandths, C = round(cutoff * 1000)."""
    C = int(round(cutoff * 1000.0))
    assert 1 <= C <= 30000
    d2 = np.zeros((len(rec_t), len(lig_t)), dtype=np.int64)
    for k in range(3):
        d = rec_t[:, None, k] - lig_t[None, :, k]
        d2 += d * d
    return d2 <= C * C


class ContactsRestated(Restated):
    def __init__(self, rec_pdb, lig_pdb, rec_modes=None, lig_modes=None):
        Restated.__init__(self, rec_pdb, lig_pdb, rec_modes, lig_modes)
        self.rec_of, self.rec_ids = read_residues(rec_pdb)
        self.lig_of, self.lig_ids = read_residues(lig_pdb)

    def residue_bits(self, xyz, cutoff=5.0, rec_atoms=None):
        """Posed (or re-read) complex coordinates -> (bool per receptor residue, bool per ligand residue).
        rec_atoms: only these receptor atoms are looked at (a cheaper question on a large receptor)."""
        n_rec = len(self.rec)
        t = thousandths(xyz)
        sel = np.arange(n_rec) if rec_atoms is None else np.asarray(rec_atoms)
        near = atom_contacts(t[:n_rec][sel], t[n_rec:], cutoff)
        rec = np.zeros(len(self.rec_ids), dtype=bool)
        lig = np.zeros(len(self.lig_ids), dtype=bool)
        rec[self.rec_of[sel][near.any(axis=1)]] = True
        lig[self.lig_of[near.any(axis=0)]] = True
        return rec, lig

    def contacts(self, row, cutoff=5.0, ligand_frame=True, rec_atoms=None):
        return self.residue_bits(self.pose(row, ligand_frame), cutoff, rec_atoms)

    def batch(self, poses, cutoff=5.0):
        both = [self.contacts(p, cutoff) for p in poses]
        return np.array([r for r, _ in both]).reshape(len(poses), -1), np.array([l for _, l in both]).reshape(len(poses), -1)


def case_restated(name):
    """A golden case of tests/conftest.py's CASES as a ContactsRestated (modes when the case uses them)."""
    from conftest import case_paths
    c, d, rec, lig = case_paths(name)
    if c["use_anm"]:
        return ContactsRestated(rec, lig, np.load(os.path.join(d, "rec_nm.npy")), np.load(os.path.join(d, "lig_nm.npy")))
    return ContactsRestated(rec, lig)


def czy_contacts_restated():
    return ContactsRestated(os.path.join(CZY, "lightdock_1czy_protein.pdb"), os.path.join(CZY, "lightdock_1czy_peptide.pdb"),
                            np.load(os.path.join(CZY, "lightdock_rec.nm.npy")), np.load(os.path.join(CZY, "lightdock_lig.nm.npy")))


def bead_atoms(rs):
    return np.array([a for a, r in enumerate(rs.rec_of) if rs.rec_ids[r].split(".")[1] == "MMB"])


# ---- the checker, pinned ----------------------------------------------------------------------------------------

def test_thousandths_and_the_integer_test():
    assert list(thousandths([0.0005, -0.0004, 1.2345, -1.2346, 4.9995, -0.0, 123.4565])) == [
        int(("%.3f" % v).replace(".", "")) for v in (0.0005, -0.0004, 1.2345, -1.2346, 4.9995, -0.0, 123.4565)]
    assert thousandths([-0.0004])[0] == 0 and thousandths([2.0])[0] == 2000 and thousandths([-12.3456])[0] == -12346
    rec = np.array([[0, 0, 0]], dtype=np.int64)
    lig = np.array([[3000, 4000, 0], [3000, 4000, 1], [5000, 0, 0], [5001, 0, 0], [2000000000, 0, 0]], dtype=np.int64)
    assert list(atom_contacts(rec, lig, 5.0)[0]) == [True, False, True, False, False]
    assert list(atom_contacts(rec, lig, 4.999)[0]) == [False] * 5


def test_residues_by_the_column_rule():
    rs = czy_contacts_restated()
    assert (len(rs.rec_ids), len(rs.lig_ids)) == (168, 7)
    assert int((rs.rec_of == rs.rec_ids.index("A.SER.467")).sum()) == 6
    ab = case_restated("ab_icode")
    six = ["H.SER.52", "H.ASP.52A", "H.MET.82", "H.SER.82A", "H.SER.82B", "H.LEU.82C"]
    assert all(ab.rec_ids.count(r) == 1 for r in six)
    k = case_restated("1k4c")
    assert (len(k.rec), len(k.lig), len(k.rec_ids), len(k.lig_ids)) == (3413, 3268, 845, 428)
    assert len(bead_atoms(k)) == 453
    azp = case_restated("1azp")
    assert (len(azp.rec_ids), len(azp.lig_ids)) == (66, 16)


def test_1czy_restraint_residue_in_the_final_swarms_and_the_ranked_models():
    an = analyse_module()
    rs = czy_contacts_restated()
    ser = rs.rec_ids.index("A.SER.467")
    counts = []
    for s in range(10):
        poses, _ = an.read_gso(os.path.join(CZY, "swarm_%d" % s, "gso_100.out"))
        assert len(poses) == 200
        counts.append(sum(int(rs.contacts(p)[0][ser]) for p in poses))
    assert counts == [96, 0, 56, 55, 77, 106, 29, 8, 2, 3] and sum(counts) == 432
    entries = an.ranking(range(10), 100, base=CZY)
    assert [bool(rs.contacts(e[2])[0][ser]) for e in entries] == [True] * 6 + [False] * 5


def test_1azp_restraints_of_the_final_swarm():
    an = analyse_module()
    rs = case_restated("1azp")
    rec_cols = [rs.rec_ids.index(r) for r in ("A.TRP.24", "A.VAL.26", "A.ARG.42")]
    lig_col = rs.lig_ids.index("B.DT.13")
    poses, _ = an.read_gso(os.path.join(GOLDEN, "1azp", "swarm_0", "gso_100.out"))
    pairs = []
    for p in poses:
        rec, lig = rs.contacts(p)
        pairs.append((int(rec[rec_cols].sum()), int(lig[lig_col])))
    assert {k: pairs.count(k) for k in set(pairs)} == {(0, 1): 119, (1, 0): 13, (1, 1): 68}
    fl = filter_module()
    rec = np.array([r / 3.0 for r, _ in pairs])
    lig = np.array([float(l) for _, l in pairs])
    beads = np.zeros(200, dtype=np.int64)
    assert int(fl.keep_mask(rec, lig, beads, 0.4).sum()) == 0      # 1/3 < 0.4
    assert int(fl.keep_mask(rec, lig, beads, 0.3).sum()) == 68


def test_1k4c_beads_in_contact_at_the_starting_positions():
    rs = case_restated("1k4c")
    beads = bead_atoms(rs)
    poses = np.loadtxt(os.path.join(GOLDEN, "1k4c", "initial_positions_0.dat"))[:10, :7]
    assert [int(rs.contacts(p, rec_atoms=beads)[0].sum()) for p in poses] == [28, 33, 28, 25, 26, 34, 23, 29, 31, 31]
    full, part = rs.contacts(poses[0]), rs.contacts(poses[0], rec_atoms=beads)    # the cheaper question, same beads
    mmb = np.array([r.split(".")[1] == "MMB" for r in rs.rec_ids])
    assert np.array_equal(full[0][mmb], part[0][mmb]) and not part[0][~mmb].any()


# ---- filter.py's file logic -------------------------------------------------------------------------------------

def test_restraints_list_parsing():
    fl = filter_module()
    text = "R A.SER.467 A\n\nL B.DT.13\nR A.LYS.1 P\n   \nR A.GLY.2 B\nL B.DA.7 P\n"
    assert fl.parse_restraints_list(text) == {"rec": ["A.SER.467", "A.LYS.1"], "lig": ["B.DT.13", "B.DA.7"]}
    assert fl.parse_restraints_list(open(os.path.join(CZY, "restraints.list")).read()) == {"rec": ["A.SER.467"], "lig": []}
    for bad in ("X A.SER.1\n", "R\n", "R A.SER.1 Q\n", "R A.SER.1 A extra\n"):
        with pytest.raises(ValueError):
            fl.parse_restraints_list(bad)
    setup = {"receptor_restraints": {"active": ["A.SER.467"], "blocked": ["A.GLY.1"], "passive": ["A.LYS.2"]},
             "ligand_restraints": {"active": [], "passive": []}}
    assert fl.setup_restraints(setup) == {"rec": ["A.SER.467", "A.LYS.2"], "lig": []}
    assert fl.setup_restraints({}) == {"rec": [], "lig": []}


def test_restraint_columns_and_fractions():
    fl = filter_module()
    residues = ["A.GLY.1", "A.SER.2", "A.MMB.3", "A.SER.2", "A.MMB.4"]     # A.SER.2 is two runs
    assert fl.restraint_columns(["A.SER.2", "A.GLY.1"], residues, "receptor") == [[1, 3], [0]]
    with pytest.raises(ValueError, match="A.TRP.9"):
        fl.restraint_columns(["A.GLY.1", "A.TRP.9"], residues, "receptor")
    contact = np.array([[1, 0, 1, 0, 1], [0, 0, 0, 1, 0], [0, 0, 0, 0, 0]], dtype=bool)
    cols = fl.restraint_columns(["A.SER.2", "A.GLY.1"], residues, "receptor")
    assert list(fl.fractions(contact, cols)) == [0.5, 0.5, 0.0]
    assert list(fl.fractions(contact, [])) == [-1.0, -1.0, -1.0]            # a side without restraints
    assert list(fl.bead_counts(contact, residues)) == [2, 0, 0]
    rec, lig = fl.fractions(contact, cols), fl.fractions(contact, [])
    beads = fl.bead_counts(contact, residues)
    assert list(fl.keep_mask(rec, lig, beads, 0.4)) == [True, True, False]
    assert list(fl.keep_mask(rec, lig, beads, 0.4, max_beads=1)) == [False, True, False]
    assert list(fl.keep_mask(rec, lig, beads, 0.6)) == [False, False, False]
    assert list(fl.keep_mask(lig, lig, beads, 0.4, max_beads=0)) == [False, True, True]


def two_swarm_run(base):
    """gso_5.out of swarms 0 and 3, three glowworms each, with ties in scoring inside a swarm and across the two."""
    header = "#Coordinates  RecID  LigID  Luciferin  Neighbor's number  Vision Range  Scoring\n"
    scores = {0: [1.5, 7.25, 1.5], 3: [7.25, -2.0, 1.5]}
    for s, sc in scores.items():
        os.makedirs(base / ("swarm_%d" % s))
        with open(base / ("swarm_%d" % s) / "gso_5.out", "w") as f:
            f.write(header + "".join("(%d.0, %d.5, 0.0, 1.0, 0.0, 0.0, 0.0)    0    0   1.00000000  0 0.200 %.8f\n" % (s, g, v)
                                     for g, v in enumerate(sc)))


def test_ordering_ties_and_the_text_of_rank_filtered_list(tmp_path):
    fl = filter_module()
    two_swarm_run(tmp_path)
    entries = fl.all_glowworms([3, 0], 5, base=str(tmp_path))
    assert [(e[0], e[1]) for e in entries] == [(0, 1), (3, 0), (0, 0), (0, 2), (3, 2), (3, 1)]
    assert list(entries[1][2]) == [3.0, 0.5, 0.0, 1.0, 0.0, 0.0, 0.0]
    rec = np.array([1.0, 0.5, -1.0, 1 / 3.0, 0.0, 2 / 3.0])
    lig = np.array([-1.0, 1.0, -1.0, 0.0, 0.25, 1.0])
    beads = np.array([0, 12, 3, 0, 0, 453])
    keep = np.array([True, True, False, True, False, True])
    assert fl.rank_filtered_text(entries, rec, lig, beads, keep) == (
        "Swarm  Glowworm     Scoring      Rec      Lig   Beads\n"
        "    0         1     7.25000    1.000   -1.000       0\n"
        "    3         0     7.25000    0.500    1.000      12\n"
        "    0         2     1.50000    0.333    0.000       0\n"
        "    3         1    -2.00000    0.667    1.000     453\n")
    assert fl.rank_filtered_text(entries, rec, lig, beads, np.zeros(6, dtype=bool)) == fl.FILTER_HEADER
