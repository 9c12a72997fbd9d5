"""The batch block of dfire_bm_pairs (csrc/kernels/dfire_bm_batch.inc, written by tools/gen_bm_batch_asm.py: schedule()) at
the smallest shapes at which a schedule of its 64 pair slots can still go wrong (run with -m gpu on an MI355X).

A schedule moves instructions; what it can break is what an instruction carries as a CONSTANT or a FIXED REGISTER: the
row of the cube a slot's table read addresses, the half of the ligand pair register its E takes (op_sel), the sum its
value is added to, the set of temporaries a granule's reads land in, and the count of every wait.  The molecules are
made so that each of these shows in a sum:

  receptor  72 atoms = one full tile of 64 + one subtile, ligand 20 atoms = two full subtiles + one of 4 atoms and 4
            padding atoms.  EVERY atom of a molecule has a type of its own (whole residues of different kinds: a DFIRE
            type is a residue's atom), so the 64 rows of every 8 x 8 block are 64 different rows of the table, whatever
            order the host gives the atoms.  (random_rigid_case draws residues at random -- types repeat inside a block,
            and from 64 receptor atoms on it adds three membrane beads --, hence the molecules of this file; its poses'
            recipe, the dyadic tables and the exactness argument are tests/test_gpu_dfire_tables.py's.)
  poses     130 = two full batches of 64 lanes + 2 lanes and 62 fillers; the molecules are small enough (boxes of 10 and
            6 A) that at the first hundred poses every pair is inside the cutoff: all 64 slots of every block add a table
            value, none the row's "miss" slot.
  tables    ladder_table(10, 2^-20): every entry an independent random multiple of 2^-20, so the oracle's f64 sum is exact
            and the kernel owes it bit for bit.  A slot that read another row (a wrong row constant), or formed its cell
            from the other atom of the pair register (a wrong op_sel half: another distance, so another bin, of another
            type pair), adds another independent entry: the pose's sum moves by a random multiple of 2^-20, and stays
            only if that multiple is 0 (one chance in 2^24 per misplaced slot).  A read that landed in a register
            still in use, or a wait one read short, does the same to two slots at once.
            constant_table(+1024): what the PARTITION of the two running sums shows in.  A value is 2^44 fixed-point
            units, a sum's marker field starts at 2^51 and is taken off by rounding at 2^50 (finish_batch): 32 values
            are 2^49, under it, and the energy cannot tell which of the two sums a SINGLE value went to (their total is
            one number) -- but the generator assigns sums by a rule (slot k of a granule: k % 2), so what a mistake
            moves is a class of slots: 16 or 32 more values in one sum are 2^49 + 2^48 or 2^50, the rounding takes
            them for a marker, and the pose's sum is off by 2^51 units.  With every pair inside the cutoff each block
            of full subtiles does hold 64 values.
"""
import numpy as np
import pytest

from test_gpu_dfire_tables import (ROUTES, BM, Case, constant_table, hold_dyadic, ladder_table, oracle_rows,
                                   random_anm_case)
from test_gpu_parity import REL_TOL, _write_pdb, bm_err

pytestmark = pytest.mark.gpu

BM_ROUTE = ROUTES[:1]
assert BM_ROUTE[0][1] == BM

# whole residues, no kind twice in a molecule: 14 + 12 + 11 + 11 + 10 + 9 + 5 = 72 and 9 + 8 + 3 = 20 atoms of different types
_RESIDUES = {
    "TRP": ["N", "CA", "C", "O", "CB", "CG", "CD1", "CD2", "CE2", "NE1", "CE3", "CZ3", "CH2", "CZ2"],
    "TYR": ["N", "CA", "C", "O", "CB", "CG", "CD1", "CD2", "CE1", "CE2", "CZ", "OH"],
    "ARG": ["N", "CA", "C", "O", "CB", "CG", "CD", "NE", "CZ", "NH1", "NH2"],
    "PHE": ["N", "CA", "C", "O", "CB", "CG", "CD1", "CD2", "CE1", "CE2", "CZ"],
    "HIS": ["N", "CA", "C", "O", "CB", "CG", "ND1", "CD2", "CE1", "NE2"],
    "GLU": ["N", "CA", "C", "O", "CB", "CG", "CD", "OE1", "OE2"],
    "ALA": ["N", "CA", "C", "O", "CB"],
    "GLN": ["N", "CA", "C", "O", "CB", "CG", "CD", "OE1", "NE2"],
    "MET": ["N", "CA", "C", "O", "CB", "CG", "SD", "CE"],
    "PRO": ["N", "CA", "C"],
}
REC_RESIDUES = ["TRP", "TYR", "ARG", "PHE", "HIS", "GLU", "ALA"]
LIG_RESIDUES = ["GLN", "MET", "PRO"]


def _typed_molecule(rng, residues, chain, box, n_atoms=None):
    """The residues' atoms at uniform positions in a box (a side per axis), every atom of another type."""
    box = np.broadcast_to(np.asarray(box, dtype=np.float64), (3,))
    atoms = []
    for seq, res in enumerate(residues, 1):
        for a in _RESIDUES[res]:
            x, y, z = np.round(rng.uniform(-box / 2, box / 2), 3)
            atoms.append((a, res, chain, seq, x, y, z))
    atoms = atoms[:n_atoms]
    assert len({(a[1], a[0]) for a in atoms}) == len(atoms)
    return atoms


def _poses(rng, n, near, reach_near, reach_far):
    """random_rigid_case's recipe: translations in a cube, quaternions of norms 0.5 .. 2; the first `near` close by."""
    poses = np.zeros((n, 7))
    poses[:, :3] = rng.uniform(-reach_far, reach_far, (n, 3))
    poses[:near, :3] = rng.uniform(-reach_near, reach_near, (near, 3))
    q = rng.normal(size=(n, 4))
    poses[:, 3:] = q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (n, 1))
    return poses


def typed_case(tmp_path, restraints):
    rng = np.random.default_rng(72020)
    rec, lig = str(tmp_path / "rec.pdb"), str(tmp_path / "lig.pdb")
    rec_atoms = _typed_molecule(rng, REC_RESIDUES, "A", 10.0)
    lig_atoms = _typed_molecule(rng, LIG_RESIDUES, "B", 6.0)
    assert len(rec_atoms) == 72 and len(lig_atoms) == 20
    _write_pdb(rec, rec_atoms)
    _write_pdb(lig, lig_atoms)
    # 100 poses with every pair inside the cutoff (half diagonals 8.7 + 5.2 A, + sqrt(3) x 0.6 < 15), 30 that cut the molecules apart
    poses = _poses(rng, 130, 100, 0.6, 9.0)
    kw = dict(rec_active=["A.ARG.3", "A.ALA.7"], lig_active=["B.MET.2"]) if restraints else {}
    return Case("typed 72x20%s" % (" restrained" if restraints else ""), rec, lig, kw, poses)


def test_every_slot_reads_its_own_row_and_adds_to_its_own_sum(pkg, orc, tmp_path):
    """Row constants, operand halves, the sums' partition, the fillers of a part-filled batch: the module docstring's case.
    Energies within the tail's roundings of the oracle's exact sums, pair counts equal (hold_dyadic)."""
    pkg.init(0)
    case = typed_case(tmp_path, False)
    _, stats = hold_dyadic(pkg, orc, case, ladder_table(10.0, 20, case.used(orc)), 20, "schedule", "vmax 10", routes=BM_ROUTE)
    assert np.all(stats[:100, 5] == 72 * 20), "the near poses hold every pair: 64 table values per block of full subtiles"
    assert 0 < stats[100:, 5].min() < 0.7 * 72 * 20, "the far poses cut the molecules apart: slots beyond the cutoff among the others"
    _, stats = hold_dyadic(pkg, orc, case, constant_table(1024.0), 0, "schedule", "+1024", routes=BM_ROUTE,
                           known_raw=lambda count: 1024.0 * count)
    assert np.array_equal(stats[:, 0], 1024.0 * stats[:, 5])


def test_flagged_cells_and_interface_flags(pkg, orc, tmp_path):
    """The same molecules with restraints: the blocks of the restrained residues' atoms are tracked (markers in the bins of
    the interface distance as well), and among 130 x 1440 pairs thousands lie in cells that hold a bin step or the cutoff and
    go through the exact path -- one marker or several in a lane's sum.  Energies (the restraint terms of the tail are the
    interface flags), and pair counts, equal the oracle's."""
    pkg.init(0)
    case = typed_case(tmp_path, True)
    _, stats = hold_dyadic(pkg, orc, case, ladder_table(10.0, 20, case.used(orc)), 20, "schedule", "vmax 10, restrained", routes=BM_ROUTE)
    assert stats[:, 2].max() > 0.0 and stats[:, 3].max() > 0.0, "restraints of both molecules are met by some pose"
    assert len(set(stats[:, 2])) > 1, "... and not by every pose alike"
    hold_dyadic(pkg, orc, case, constant_table(1024.0), 0, "schedule", "+1024, restrained", routes=BM_ROUTE,
                known_raw=lambda count: 1024.0 * count)


def test_posing_in_halves(pkg, orc, tmp_path):
    """A ligand of 18 atoms strung along 44 A: its last subtile holds 2 atoms and 6 padding atoms -- padding in both halves
    (atoms 0-3 and 4-7) of the lane's posed operands --, and poses that carry it along its own axis across the edge of the
    f32 frame (the receptor + 16 A) leave subtiles with some atoms inside the frame and some outside."""
    pkg.init(0)
    rng = np.random.default_rng(18044)
    rec, lig = str(tmp_path / "rec.pdb"), str(tmp_path / "lig.pdb")
    _write_pdb(rec, _typed_molecule(rng, REC_RESIDUES, "A", 10.0))
    _write_pdb(lig, _typed_molecule(rng, LIG_RESIDUES, "B", (44.0, 4.0, 4.0), n_atoms=18))
    poses = _poses(rng, 70, 10, 2.0, 12.0)
    poses[10:60, 3:] = [1.0, 0.0, 0.0, 0.0]                      # the ligand's long axis stays x ...
    poses[10:60, 0] = np.linspace(-45.0, 45.0, 50)               # ... and crosses both edges of the frame atom by atom
    poses[10:60, 1:3] = rng.uniform(-3.0, 3.0, (50, 2))
    case = Case("typed 72x18, a strung-out ligand", rec, lig, {}, poses)
    _, stats = hold_dyadic(pkg, orc, case, ladder_table(10.0, 20, case.used(orc)), 20, "schedule", "vmax 10", routes=BM_ROUTE)
    assert stats[10:60, 5].min() == 0 and stats[10:60, 5].max() > 200, "from out of reach to across the receptor"


def test_anm_form(pkg, orc, table, tmp_path):
    """The block with its receptor operands in vector registers (LD_BM_BATCH_ASM_V): 70 poses, one of them wild."""
    pkg.init(0)
    case = random_anm_case(tmp_path, 72, 20, 3, 3, False)
    rng = np.random.default_rng(7020)
    poses = case.poses[np.arange(70) % len(case.poses)].copy()
    poses[:, :3] += rng.uniform(-1.0, 1.0, (70, 3))
    poses[:, 7:] = rng.normal(size=(70, 6)) * 2.0
    poses[33, 7:] *= 40.0
    want, _ = oracle_rows(case.cpu(orc, table), poses)
    hip = case.hip(pkg, table)
    assert hip.kernel_info()["pair_kernel_name"] == BM
    got = hip.energy_batch(poses)
    print("ANM form, 70 poses: bm_err %.3e" % bm_err(got, want))
    assert bm_err(got, want) < REL_TOL
