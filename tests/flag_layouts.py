"""Lattice complexes that move the interface-flag layer -- one bit ("slot") per restraint atom and per membrane bead in a pose's
flag words (scorer.cpp: slot_molecule), read by satisfied_fraction and membrane_beads (kernels/pose_energy_tail.hpp) -- off its
smallest layouts: a second and later flag word on either side, groups that straddle a word boundary, a side with no words, every
block tracked, and every entry and exit of membrane_beads' four-trip loop.  Shared by tests/test_flag_layouts_cpu.py (the oracle
alone: the coverage is realised) and tests/test_gpu_flag_layouts.py (every pair route against the oracle).  No test functions here.

Lattice.  8 cells a row, 6 A apart, in the plane z = 0; cell k sits at (6 (k % 8), 6 (k // 8), 0).  A RESIDUE cell is an ALA:
N, CA, C, O at (+-0.5, +-0.5, 0) and CB at (0, 0, -0.7) around the cell's centre; a BEAD cell is one MMB / BJ atom (chain M) at the
centre.  The receptor (chain A) is `n_rec` residue cells followed by `beads` bead cells, the ligand (chain B) `n_lig` residue
cells.  `every` in {1, 2}: the residue cells 0, every, 2 every, ... of a side are its active restraints, five slots a group in
atom order, the beads' slots after them -- with every = 2 a bit that lands in a neighbour's slot shows.  `sides` names what is
tracked at all: "both", "rec" or "lig" (restraints of that side only, no beads), "beads" (beads only), "none".

Poses.  The identity rotation and the translation (6 a, 6 b, 1.6) for all a in [-8, 8], b in [-rows, rows], rows =
ceil(n_lig / 8) (the receptor's rows where it is the longer side: the one-cell ligand of "onehot-rec"), then one pose at
z = 40 where nothing is in range.  At z = 1.6 a ligand cell over a receptor cell has every atom pair within 2.41 A (N over the other cell's CB: sqrt(0.5 + 2.3^2)), inside DFIRE's interface distance of 2.45 A
(2 r - 1 <= 3.9, src/dfire.rs:339) and DNA's of 3.9 A; atoms of neighbouring cells are at least 5 A apart.  A shift (a, b) selects
a rectangle of touching cells, from one cell at the corners to the full overlap at (0, 0).  The oracle is the truth for every
pose; the construction only has to realise the coverage tests/test_flag_layouts_cpu.py asks for.

ANM form.  One receptor mode that moves every atom by (6, 0, 0) per unit amplitude and one ligand mode of (0, 6, 0): the shift
(a, b) of every pose above is split into a multiple of 5 cells in the translation and the rest, in {0, +-1, +-2}, in the
amplitudes (the receptor's is -rest of a: moving the receptor one cell right is the ligand one cell left).  Six more poses carry
amplitudes of +-8 -- 48 A, WILD for the block-major ANM form (beyond 16 A a coordinate) -- with the translation making up for them.

Zero table.  With potential = 0 the DFIRE pair sum is 0.0 in any order and the energy is 4.7 + pr 4.7 + pl 4.7 - penalty, a
function of the flags alone (`closed_form`): the oracle and every GPU route must agree bit for bit.  Every receptor subtile is
then "quiet" (scorer.cpp: bm_box_reaches): a block is listed through the interface reach only, and only because something is
tracked.
"""
import os

import numpy as np

from test_gpu_parity import _write_pdb

COLS, PITCH, Z_TOUCH, Z_FAR = 8, 6.0, 1.6, 40.0
ALA = (("N", 0.5, 0.5, 0.0), ("CA", 0.5, -0.5, 0.0), ("C", -0.5, 0.5, 0.0), ("O", -0.5, -0.5, 0.0), ("CB", 0.0, 0.0, -0.7))
ATOMS_PER_CELL = len(ALA)
TABLE_LEN = 169 * 169 * 20

# name -> (n_rec, beads, n_lig, every, sides, anm)
LAYOUTS = {}
for _spec in ((1, 1, 2, 1), (13, 7, 20, 2), (32, 9, 41, 1), (33, 25, 58, 2), (65, 33, 98, 1), (64, 64, 128, 2)):
    LAYOUTS["%d-%d-%d-e%d" % _spec] = _spec + ("both", False)
BEAD_LADDER = (8, 24, 31, 32, 57, 65)
for _beads in BEAD_LADDER:
    LAYOUTS["ladder-%d" % _beads] = (7, _beads, _beads + 7, 1, "both", False)
LAYOUTS["onehot-rec"] = (33, 25, 1, 2, "both", False)
LAYOUTS["onehot-lig"] = (1, 0, 65, 2, "both", False)
LAYOUTS["rec-only"] = (13, 0, 20, 1, "rec", False)
LAYOUTS["lig-only"] = (13, 0, 20, 2, "lig", False)
LAYOUTS["beads-only"] = (13, 7, 20, 1, "beads", False)
LAYOUTS["nothing-named"] = (13, 0, 20, 1, "none", False)
LAYOUTS["33-25-58-e2-anm"] = (33, 25, 58, 2, "both", True)
FULL = tuple(n for n in LAYOUTS if not n.startswith("onehot"))      # the layouts whose poses reach every count (the CPU suite)
ANM_REST = 2                                                       # the amplitudes carry a shift's remainder in [-2, 2]
WILD_AMPLITUDE = 8.0
WILD_SHIFTS = ((0, 0), (1, 0), (-3, 2), (7, -1), (-7, 3), (2, -4))


def cell_xy(k):
    return PITCH * (k % COLS), PITCH * (k // COLS)


def residue_cell(chain, k):
    x, y = cell_xy(k)
    return [(name, "ALA", chain, k + 1, x + dx, y + dy, dz) for name, dx, dy, dz in ALA]


def bead_cell(k):
    x, y = cell_xy(k)
    return [("BJ", "MMB", "M", k + 1, x, y, 0.0)]


def molecule_atoms(chain, n_cells, beads=0):
    atoms = []
    for k in range(n_cells):
        atoms.extend(residue_cell(chain, k))
    for k in range(n_cells, n_cells + beads):
        atoms.extend(bead_cell(k))
    return atoms


def named(chain, n_cells, every):
    return ["%s.ALA.%d" % (chain, k + 1) for k in range(0, n_cells, every)]


def closed_form(stats):
    """The zero-table energy from the oracle's own fractions, in the reference's order (src/dfire.rs:347-361)."""
    stats = np.atleast_2d(stats)
    score = (0.0 * 0.0157 - 4.7) * -1.0
    penalty = np.where(stats[:, 4] > 0.0, 999.0 * stats[:, 4], 0.0)
    return score + stats[:, 2] * score + stats[:, 3] * score - penalty


class Layout:
    """One lattice complex, made once and left unchanged: the PDB files, the keyword arguments both scorers take (without the
    potential), the poses with their shifts, and the oracle's energies and stats under both tables ("zero", "synth")."""

    def __init__(self, orc, table, directory, name):
        self.name = name
        self.n_rec, self.beads, self.n_lig, self.every, self.sides, self.anm = LAYOUTS[name]
        self.rec_atoms = molecule_atoms("A", self.n_rec, self.beads if self.sides in ("both", "beads") else 0)
        self.lig_atoms = molecule_atoms("B", self.n_lig)
        self.n_beads = self.beads if self.sides in ("both", "beads") else 0
        self.rec_pdb, self.lig_pdb = os.path.join(directory, name + "_rec.pdb"), os.path.join(directory, name + "_lig.pdb")
        _write_pdb(self.rec_pdb, self.rec_atoms)
        _write_pdb(self.lig_pdb, self.lig_atoms)
        self.rec_active = named("A", self.n_rec, self.every) if self.sides in ("both", "rec") else []
        self.lig_active = named("B", self.n_lig, self.every) if self.sides in ("both", "lig") else []
        self.n_rec_groups, self.n_lig_groups = len(self.rec_active), len(self.lig_active)
        self.kwargs = dict(rec_active=self.rec_active, lig_active=self.lig_active)
        if self.anm:
            rec_mode, lig_mode = np.zeros((1, len(self.rec_atoms), 3)), np.zeros((1, len(self.lig_atoms), 3))
            rec_mode[0, :, 0], lig_mode[0, :, 1] = PITCH, PITCH
            self.kwargs.update(use_anm=True, rec_nmodes=rec_mode, rec_num_anm=1, lig_nmodes=lig_mode, lig_num_anm=1)
        self.rows = -(-max(self.n_lig, self.n_rec + self.beads) // COLS)
        self.shifts = [(a, b) for a in range(-COLS, COLS + 1) for b in range(-self.rows, self.rows + 1)]
        self.wild = []
        rows = [self._pose(a, b) for a, b in self.shifts]
        if self.anm:
            for a, b in WILD_SHIFTS:
                self.wild.append(len(rows))
                self.shifts.append((a, b))
                rows.append(self._pose(a, b, wild=True))
        self.shifts.append(None)                                    # the pose where nothing is in range
        far = self._pose(0, 0)
        far[2] = Z_FAR
        rows.append(far)
        self.poses = np.ascontiguousarray(np.array(rows))
        self.tables = {"zero": np.zeros(TABLE_LEN), "synth": np.asarray(table, dtype=np.float64)}
        self.cpu, self.energy, self.stats = {}, {}, {}
        for which, potential in self.tables.items():
            self.cpu[which] = orc.Scorer("dfire", self.rec_pdb, self.lig_pdb, potential=potential, **self.kwargs)
            ex = [self.cpu[which].energy_ex_row(p) for p in self.poses]
            self.energy[which] = np.array([e for e, _ in ex])
            self.stats[which] = np.array([s for _, s in ex])
        for arr in [self.poses] + list(self.energy.values()) + list(self.stats.values()) + list(self.tables.values()):
            arr.setflags(write=False)

    def _pose(self, a, b, wild=False):
        if not self.anm:
            return np.array([PITCH * a, PITCH * b, Z_TOUCH, 1.0, 0.0, 0.0, 0.0])
        if wild:
            rest_a, rest_b = (-WILD_AMPLITUDE if a % 2 else WILD_AMPLITUDE), (WILD_AMPLITUDE if b % 2 else -WILD_AMPLITUDE)
        else:
            rest_a, rest_b = ((a + ANM_REST) % 5) - ANM_REST, ((b + ANM_REST) % 5) - ANM_REST
        return np.array([PITCH * (a - rest_a), PITCH * (b - rest_b), Z_TOUCH, 1.0, 0.0, 0.0, 0.0, -float(rest_a), float(rest_b)])

    def hits(self, which="zero"):
        """(receptor groups hit, ligand groups hit, beads flagged) per pose, as the oracle's fractions say."""
        s = self.stats[which]
        return (np.rint(s[:, 2] * self.n_rec_groups).astype(np.int64), np.rint(s[:, 3] * self.n_lig_groups).astype(np.int64),
                np.rint(s[:, 4] * self.n_beads).astype(np.int64))

    def label(self, i):
        shift = self.shifts[int(i)]
        return "%s pose %d %s" % (self.name, i, "far (z = 40)" if shift is None else "shift (a, b) = (%d, %d)%s" % (
            shift[0], shift[1], " wild" if int(i) in self.wild else ""))

    def counts_implied(self, energy):
        """The (receptor hits, ligand hits, beads) whose zero-table energy is `energy` bit for bit; [] if there are none."""
        hr, hl, nb = np.meshgrid(np.arange(self.n_rec_groups + 1), np.arange(self.n_lig_groups + 1), np.arange(self.n_beads + 1), indexing="ij")
        stats = np.zeros((hr.size, 8))
        stats[:, 2] = hr.ravel() / max(self.n_rec_groups, 1)
        stats[:, 3] = hl.ravel() / max(self.n_lig_groups, 1)
        stats[:, 4] = nb.ravel() / max(self.n_beads, 1)
        at = np.flatnonzero(closed_form(stats) == energy)
        return [(int(hr.ravel()[k]), int(hl.ravel()[k]), int(nb.ravel()[k])) for k in at[:4]]


_CACHE = {}


def layout(orc, table, directory, name):
    if name not in _CACHE:
        _CACHE[name] = Layout(orc, table, directory, name)
    return _CACHE[name]


# ---- the DNA / PYDOCK all-pairs kernel on the same lattices --------------------------------------------------------------------

DNA_LATTICES = {"33-25-58-e2": (33, 25, 58, 2), "7-32-39-e1": (7, 32, 39, 1)}
DNA_CHUNK = 64                  # LIGHTDOCK_CHUNK_ATOMS: 190 receptor atoms in 3 chunks, 67 in 2 -- flags of different chunks OR together
_DNA_CACHE = {}


def _xyz(atoms):
    return np.array([a[4:7] for a in atoms], dtype=np.float64)


def dna_case(orc, name):
    """A lattice as ld_molecule arrays for Scorer.from_arrays: charges and radii from dna_reference.synthetic's generator, the
    restraint CSR and the bead list as the PDB route would give them (groups in residue order, five atoms each; the beads after
    the residues).  Poses: the lattice shifts and the far pose (three trailing columns as dna_reference's rows have).
    -> (rec, lig, poses, shifts, references, shape for tests/test_gpu_dna_pairs.py::build)."""
    if name not in _DNA_CACHE:
        import dna_reference as dr
        n_rec, beads, n_lig, every = DNA_LATTICES[name]
        rec_xyz, lig_xyz = _xyz(molecule_atoms("A", n_rec, beads)), _xyz(molecule_atoms("B", n_lig))
        rec, lig = dr.synthetic(len(rec_xyz), len(lig_xyz), 1000 * n_rec + n_lig)
        rec["coordinates"], lig["coordinates"] = rec_xyz, lig_xyz
        for mol, cells in ((rec, n_rec), (lig, n_lig)):
            groups = list(range(0, cells, every))
            mol["restraint_offsets"] = (ATOMS_PER_CELL * np.arange(len(groups) + 1)).astype(np.uint32)
            mol["restraint_atoms"] = np.concatenate([np.arange(ATOMS_PER_CELL * k, ATOMS_PER_CELL * (k + 1)) for k in groups]).astype(np.uint32)
        rec["membrane"] = (ATOMS_PER_CELL * n_rec + np.arange(beads)).astype(np.uint32)
        rows_lig = -(-n_lig // COLS)
        shifts = [(a, b) for a in range(-COLS, COLS + 1) for b in range(-rows_lig, rows_lig + 1)] + [None]
        poses = np.full((len(shifts), 10), np.nan)
        poses[:, 3:7] = (1.0, 0.0, 0.0, 0.0)
        for p, shift in enumerate(shifts):
            poses[p, :3] = (0.0, 0.0, Z_FAR) if shift is None else (PITCH * shift[0], PITCH * shift[1], Z_TOUCH)
        n_chunks = -(-len(rec_xyz) // DNA_CHUNK)
        want = [dr.dna_reference(orc, rec, lig, row, n_chunks=n_chunks) for row in poses]
        _DNA_CACHE[name] = (rec, lig, poses, shifts, want, (len(rec_xyz), len(lig_xyz), DNA_CHUNK, n_chunks))
    return _DNA_CACHE[name]
