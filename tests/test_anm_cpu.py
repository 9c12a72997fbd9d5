"""Normal modes, the part that needs no GPU: which atom is a residue's node (ld_anm_nodes, host only), the refusal that
names a residue without one, and the yardstick itself -- tests/anm_reference.py, the rule of lightdock_hip.h "Normal modes"
in numpy, must reproduce the mode files under tests/golden that ProDy wrote, up to each mode's sign."""
import os

import numpy as np
import pytest

import anm_reference as ar
from conftest import GOLDEN

# molecule -> (PDB, mode file, atoms, nodes, node atom)
MOLECULES = {
    "2uuy_rec": ("2uuy/lightdock_2UUY_rec.pdb", "2uuy/rec_nm.npy", 1615, 220, "CA"),
    "2uuy_lig": ("2uuy/lightdock_2UUY_lig.pdb", "2uuy/lig_nm.npy", 415, 55, "CA"),
    "1azp_rec": ("1azp/lightdock_protein.pdb", "1azp/rec_nm.npy", 1094, 66, "CA"),
    "1azp_dna": ("1azp/lightdock_dna.pdb", "1azp/lig_nm.npy", 506, 16, "C4'"),
    "ab_icode_rec": ("ab_icode/lightdock_receptor.pdb", "ab_icode/rec_nm.npy", 3326, 437, "CA"),
    "1czy_rec": ("1czy/lightdock_1czy_protein.pdb", "1czy/rec_nm.npy", 1281, 168, "CA"),
    "1czy_lig": ("1czy/lightdock_1czy_peptide.pdb", "1czy/lig_nm.npy", 53, 7, "CA"),
}
SCALED = ("1czy_rec", "1czy_lig")   # written with anm_rec_rmsd / anm_lig_rmsd: c / sqrt(lambda_k) times the unit mode


def golden_modes(name):
    pdb, npy, atoms, _, _ = MOLECULES[name]
    return np.load(os.path.join(GOLDEN, npy)).reshape(10, atoms, 3)


@pytest.mark.parametrize("name", sorted(MOLECULES))
def test_node_atoms_of_the_golden_molecules(pkg, name):
    pdb, _, atoms, nodes, atom = MOLECULES[name]
    path = os.path.join(GOLDEN, pdb)
    got = pkg.anm_nodes(path)
    names, keys, _ = ar.read_pdb(path)
    res = ar.residues(keys)
    assert len(names) == atoms and got.shape == (nodes,) and got.dtype == np.uint32
    assert {names[a] for a in got} == {atom}
    assert np.array_equal(res[got], np.arange(nodes))           # one a residue, in file order
    assert np.array_equal(got, ar.node_atoms(names, res))       # the FIRST such atom of the residue
    if name == "ab_icode_rec":                                  # residues that differ in the insertion code alone are nodes of their own
        ids = [ar.residue_id(keys[a]) for a in got]
        assert len(set(ids)) == nodes and {"H.ASP.52A", "H.LEU.82C"} <= set(ids)


def test_a_residue_without_a_node_atom_is_named(pkg, tmp_path):
    lines = open(os.path.join(GOLDEN, "1czy", "lightdock_1czy_peptide.pdb")).read().splitlines(True)
    names, keys, _ = ar.read_pdb(os.path.join(GOLDEN, "1czy", "lightdock_1czy_peptide.pdb"))
    res = ar.residues(keys)
    victim = 3
    atoms = [l for l in lines if l.startswith("ATOM  ") or l.startswith("HETATM")]
    kept = [l for a, l in enumerate(atoms) if not (res[a] == victim and names[a] == "CA")]
    path = tmp_path / "no_ca.pdb"
    path.write_text("".join(kept))
    want = ar.residue_id(keys[int(np.nonzero(res == victim)[0][0])])
    with pytest.raises(pkg.LightdockError) as e:
        pkg.anm_nodes(str(path))
    assert e.value.status == -1 and want in str(e.value)
    # a membrane bead has no node atom either
    with pytest.raises(pkg.LightdockError) as e:
        pkg.anm_nodes(os.path.join(GOLDEN, "1k4c", "lightdock_receptor_membrane.pdb"))
    assert e.value.status == -1 and "MMB" in str(e.value)
    with pytest.raises(pkg.LightdockError) as e:
        pkg.anm_nodes(str(tmp_path / "no_such.pdb"))
    assert e.value.status == -3


@pytest.mark.parametrize("name", sorted(MOLECULES))
def test_the_numpy_restatement_reproduces_the_golden_modes(name):
    """Up to sign, 1e-13 absolute where the golden holds unit modes; 1e-11 after the one scale a mode where it holds scaled
    ones, and that scale is c / sqrt(lambda_k) with one c for all ten modes."""
    pdb = MOLECULES[name][0]
    lam, want = ar.atom_modes(os.path.join(GOLDEN, pdb), 10)
    gold = golden_modes(name)
    if name not in SCALED:
        for r in range(10):
            assert np.abs(ar.align(gold[r], want[r]) - want[r]).max() < 1e-13, r
        return
    c = []
    for r in range(10):
        scale = np.sqrt((gold[r] ** 2).sum())
        assert np.abs(ar.align(gold[r] / scale, want[r]) - want[r]).max() < 1e-11, r
        c.append(scale * np.sqrt(lam[r]))
    assert np.ptp(c) < 1e-9 * c[0]
    assert abs(c[0] - {"1czy_rec": 3.06678976, "1czy_lig": 0.54155563}[name]) < 1e-7


def test_bounds_of_the_golden_set():
    """The loosest eigenvector bound over the golden molecules stays far below a mode's components."""
    worst = 0.0
    for name, (pdb, _, _, _, _) in MOLECULES.items():
        names, keys, xyz = ar.read_pdb(os.path.join(GOLDEN, pdb))
        nodes = ar.node_atoms(names, ar.residues(keys))
        w = np.linalg.eigvalsh(ar.hessian(xyz[nodes]))
        assert np.abs(w[:6]).max() < 1e-12 and w[6] > 1e-3
        worst = max(worst, ar.bounds(w, 10)[1].max())
    assert worst < 1e-7   # against components of 0.03 .. 0.15
