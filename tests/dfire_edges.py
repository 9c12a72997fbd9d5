"""Poses that sit ON the knife edges of the DFIRE pair kernels' decisions -- the 20 bin steps, the interface distance d <= 3.9
and the cutoff d2 <= 225 (src/dfire.rs:334-339) -- for the two culled routes, the block-major `dfire_bm_*` kernels and the
pose-major `dfire_packed_pairs`.  Both decide in f32 and send a pair to their exact f64 path only where the f32 distance comes
within `eps` of a step; `eps` is derived by hand (scorer.cpp: dfire_bm_error_bound, dfire_f32_error_bound).  Shared by
tests/test_dfire_edges_cpu.py (the oracle alone: every edge is realised; and a replay of the block-major f32 arithmetic) and
tests/test_gpu_dfire_edges.py (the kernels against the oracle).  No test functions here.

The oracle is the only judge of where an edge lies: every edge is found by BISECTION ON THE ORACLE's own answer, on the bit
pattern of a scalar, down to two adjacent doubles with different answers.

Complexes.  Hand-made molecules written as PDB files.  Atom 0 of either side is the TARGET, the others are ANCHORS that set the
frame (receptor) and the extent (ligand).  In every pose of a geometry the target pair is the ONLY pair within 15 A: no other
pair comes within 15.5 A (checked here in f64, and by the oracle's in-cutoff count).  That rules a target with neighbours a few
angstrom away out -- the ligand target comes within 2 A of the receptor's -- so a "cluster" here is loose: the receptor
target's nearest neighbours are 15.9 A and more away, inward, and the ladder's direction points outward.  What the geometries
are for does not need them closer: the size of the frame, the target at the frame's corner (where the f32 ulp is largest), and the
half extent of the target's 8-atom subtile, whose box centre is the origin of the block-major distance arithmetic.
Complex "A" has no restraints (energy = 4.7 - 0.0157 v[bin]); complex "B" has the two target residues as restraints, so the
interface flag of the target pair triples the energy, and every atom of its target subtiles has an interface-flag slot.

Potential.  A STAIRCASE: value[:, :, b] = b + 1 for every pair of types (small integers: exact in the block-major fixed point;
neighbouring bins differ by 1.0, i.e. 0.0157 in the energy, seven orders above the tolerance).  STAIRCASE0 leaves the last bin
at 0.0, so that the zero-bin elision of both routes is active.  Complex A is scored with the first, complex B with the second.

Geometries (the frame sizes come from the library's own route predicates through `pkg.dfire_route_frames`, searched, not
typed in):
  G1-G4  receptor of 24 atoms: the target at the corner (2h, 2h, 2h) of its bounding cube [0, 2h]^3, 15 atoms 9.2 to 30 A inward of it on every
         axis, 8 atoms at the opposite corner; h = the largest multiple of 1/8 A at which the block-major frame is 256, 512, 1024,
         2048 record units.  The ligand's target is 59.9 A from the ligand's origin, its 15 anchors within 3 A of the origin.
  G5     the same with the largest h the block-major route still takes (the last frame with eps < 8 cells); G6: 1/8 A more,
         which it declines.
  G3anm  G3's shape under the ANM form's frame, 3 + 3 modes (below).
  W1-W4  WIDE SUBTILES: a receptor of exactly 8 atoms, i.e. one subtile: the target at (2H, 2H, 2H) with three atoms 9.2 to 12 A
         inward of it, four atoms at the origin, H = 8, 20, 40, 100 A: two groups at -+H of the subtile's centre.  dfire_bm_error_bound assumes |r - c| < 16 A for the
         rounding of r - c and |l - c| < 45 A for the operands of the distance arithmetic; H = 8 is inside that, the others are not.
The subtiles are rebuilt from `pkg.dfire_tile_layout`; the target subtile's half extent must be at most 16 A for G*, at least
0.9 H for W*.

Poses.  Per geometry 3 rotations: the identity, a random unit quaternion, a random quaternion of norm 1.7 (drawn again while
an anchor would come within 15.5 A of the other side).  Per rotation and EDGE -- 20 bin steps, the interface distance, the
cutoff -- the ligand's target is put at receptor target + rho u, u a fixed random outward direction, through the translation
t = r + rho u - q_rotate(q, x); rho is bisected between nominal -+ 0.01 A until rho0 < rho1 are adjacent doubles with different
oracle answers (energy of complex A for the bin steps, `stats[5]` for the cutoff, energy of complex B for the interface).  RUNGS:
rho0, rho1, rho0 - 2^-k and rho1 + 2^-k for k = 6, 8, .., 44: 42 poses an edge, from one ulp to beyond a LUT cell (1e-3 A at
r = 7.5).  Step 20 is the cutoff itself (r = 15): below it bin 19, above it nothing, and AT d2 == 225.0 exactly -- when a double
rho hits it -- the reference's read past the row (bin "20" = the next ligand type's bin 0).  The bisection of step 20 (on the
energy) and of the cutoff (on the count) then end on different sides of that one point; `special` marks it.

ANM (G3anm).  Mode 0 moves either target along x by its amplitude, modes 1 and 2 along y and z by half of theirs, the anchors
by hundredths; amplitudes (14.4, 1, -1.5) and (-14.4, 1.5, -1): 0.9 x 16 A on one coordinate, not WILD; the second batch has
(16.1, ..): just above 16 A, WILD, everything goes exact.  The edges are bisected with the oracle as before, per batch.

The REPLAY restates in numpy float32, operation by operation, what the block-major route computes for the target pair in the
rigid form (scorer.cpp: bm_rec_ops; dfire_bm.hip: dfire_bm_pose, the batch and bm_recheck; dfire_tiled.hip: the records and the
subtile's box): record fl32(8 (x - c_frame)), the widened box and its centre, the f32 rotation matrix and translation, three
fmas a coordinate, E = (seed - |r-c|^2) - |l-c|^2 + 2 (r-c).(l-c) in the kernel's order.  An f32 fma is emulated THROUGH F64
(product exact in f64, one f64 add, one rounding to f32: a double rounding in rare ties, 2^-29 relative at the worst, far below
what is measured here); math.fma is not used.  The pose matrix's f64 expressions are evaluated without contraction.
"""
import os

import numpy as np

from test_gpu_parity import _write_pdb

F32 = np.float32
SEED_CELL = 14583.5            # kBmCellZero + 1/2: E = SEED_CELL - 64 d2
FLAGGED, MISS = 168, 160       # codes of ld_dfire_bm_lut
BRACKET = 0.01                 # angstrom either side of an edge's nominal place
RUNG_KS = tuple(range(6, 46, 2))
N_RUNGS = 2 + 2 * len(RUNG_KS)
CLEAR = 15.5                   # angstrom: no pair but the target pair comes closer
X_LIG = (-52.137, 25.291, 16.073)   # the ligand target in the ligand's frame: 60 A from its origin; no coordinate is an f32
TARGET_INSET = np.array([0.137, 0.073, 0.191])   # the receptor target's place inside the corner: its records are no f32 either
G_UBOUNDS = {"G1": 256.0, "G2": 512.0, "G3": 1024.0, "G4": 2048.0}
W_HALF = {"W1": 8.0, "W2": 20.0, "W3": 40.0, "W4": 100.0, "W5": 400.0}
GEOMETRIES = ("G1", "G2", "G3", "G4", "G5", "W1", "W2", "W3", "W4")
ANM_AMPS = {"flex": ((14.4, 1.0, -1.5), (-14.4, 1.5, -1.0)), "wild": ((16.1, 1.0, -1.5), (-16.1, 1.5, -1.0))}
_ANCHOR_NAMES = [("N", "GLY"), ("CA", "GLY"), ("C", "GLY"), ("O", "GLY"), ("N", "SER"), ("CA", "SER"), ("CB", "SER"), ("OG", "SER")]


def staircase(table, zero_last=False):
    t = np.array(table, dtype=np.float64).reshape(169, 169, 20).copy()
    t[:, :, :] = np.arange(1.0, 21.0)
    if zero_last:
        t[:, :, 19] = 0.0
    return t.reshape(-1)


def edge_names():
    return ["step%d" % s for s in range(1, 21)] + ["interface", "cutoff"]


# ---- molecules -------------------------------------------------------------------------------------------------------------

def _atoms(chain, xyz):
    """The target as residue 1 (ALA CA), the anchors as residues 2.. (GLY / SER atoms, four a residue)."""
    out = [("CA", "ALA", chain, 1, *xyz[0])]
    for k, p in enumerate(xyz[1:]):
        name, res = _ANCHOR_NAMES[k % 8]
        out.append((name, res, chain, 2 + k // 4, *p))
    return out


def receptor_xyz(kind, h, rng):
    """Coordinates with 3 decimals (what a PDB line holds), the target first, the bounding cube [0, 2 h - TARGET_INSET] (nothing negative:
    a PDB column holds 9999.999 but not -1000.000)."""
    corner = np.array([2.0 * h, 2.0 * h, 2.0 * h]) - TARGET_INSET
    if kind == "G":
        inward = rng.uniform(9.2, min(30.0, 2.0 * h), (15, 3))
        far = np.vstack([np.zeros(3), rng.uniform(0.0, min(4.0, 2.0 * h), (7, 3))])
    else:
        inward = rng.uniform(9.2, min(12.0, 2.0 * h), (3, 3))
        far = np.vstack([np.zeros(3), rng.uniform(0.0, 3.0, (3, 3))])
    return np.round(np.vstack([corner, corner - inward, far]), 3)


def ligand_xyz(rng):
    return np.round(np.vstack([np.array(X_LIG), rng.uniform(-3.0, 3.0, (15, 3))]), 3)


def _search_h(pkg, want, lig, seed, kind="G", anm=False):
    """The largest h, a multiple of 1/8 A, for which want(block-major frame of the receptor built with h) holds (want is
    monotone: true below, false above)."""
    def ok(n):
        rec = receptor_xyz(kind, n / 8.0, np.random.default_rng(seed))
        return want(pkg.dfire_route_frames(rec, lig, anm=anm)["bm"])
    lo, hi = 80, 160   # eighths of an angstrom: h = 10 A holds for every frame asked for here
    assert ok(lo)
    while ok(hi):
        lo, hi = hi, hi * 2
        assert hi < 1 << 24
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return lo / 8.0


def _rotation(q):
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def subtile_boxes(pkg, model):
    """(lo, hi, subtile of atom 0) of a molecule's 8-atom subtiles in the scorer's order, angstrom."""
    order, _ = pkg.dfire_tile_layout(model["coordinates"], model["dfire_types"])
    pad = order == 0xFFFFFFFF
    xyz = model["coordinates"][np.where(pad, 0, order).astype(np.int64)].reshape(-1, 8, 3)
    valid = ~pad.reshape(-1, 8)
    lo = np.where(valid[..., None], xyz, np.inf).min(1)
    hi = np.where(valid[..., None], xyz, -np.inf).max(1)
    return lo, hi, int(np.flatnonzero(order == 0)[0]) // 8, order


# ---- a geometry: molecules, oracles, poses, the oracle's answers -----------------------------------------------------------------

class Geometry:
    """Everything of one geometry, made once and left unchanged.  poses[(batch)]: (3 rotations x 22 edges x 42 rungs, pose_len);
    index = (rotation * 22 + edge) * 42 + rung, rungs ordered by rho: 20 below, rho0, rho1, 20 above."""

    def __init__(self, pkg, orc, table, directory, name, seed=2024):
        self.name, self.anm, self.orc = name, name.endswith("anm"), orc
        rng = np.random.default_rng([seed, sum(map(ord, name))])
        self.lig_xyz = ligand_xyz(rng)
        rec_seed = int(rng.integers(1 << 30))
        kind = "W" if name.startswith("W") else "G"
        if name in W_HALF:
            self.h = W_HALF[name]
        elif name in ("G5", "G6"):
            self.h = _search_h(pkg, lambda f: f["takes"], self.lig_xyz, rec_seed) + (0.125 if name == "G6" else 0.0)
        else:
            u = G_UBOUNDS[name[:2]]
            self.h = _search_h(pkg, lambda f: f["ubound"] <= u, self.lig_xyz, rec_seed, anm=self.anm)
        self.rec_xyz = receptor_xyz(kind, self.h, np.random.default_rng(rec_seed))
        # the frame with every subtile inside what the bound assumes (ld_dfire_bm_lut's eps); `frames`, below: the scorer's
        self.frames_compact = pkg.dfire_route_frames(self.rec_xyz, self.lig_xyz, anm=self.anm)
        if name[:2] in G_UBOUNDS:
            assert self.frames_compact["bm"]["ubound"] == G_UBOUNDS[name[:2]], (name, self.frames_compact["bm"])
        self.rec_pdb, self.lig_pdb = os.path.join(directory, name + "_rec.pdb"), os.path.join(directory, name + "_lig.pdb")
        _write_pdb(self.rec_pdb, _atoms("A", self.rec_xyz))
        _write_pdb(self.lig_pdb, _atoms("B", self.lig_xyz))
        self.tables = {"A": staircase(table), "B": staircase(table, zero_last=True)}
        self.kwargs = {"A": dict(potential=self.tables["A"]), "B": dict(potential=self.tables["B"], rec_active=["A.ALA.1"], lig_active=["B.ALA.1"])}
        self.batches = ("flex", "wild") if self.anm else ("rigid",)
        if self.anm:
            self.rec_modes, self.lig_modes = self._modes(rng, len(self.rec_xyz)), self._modes(rng, len(self.lig_xyz))
            for kw in self.kwargs.values():
                kw.update(use_anm=True, rec_nmodes=self.rec_modes, rec_num_anm=3, lig_nmodes=self.lig_modes, lig_num_anm=3)
        self.cpu = {c: orc.Scorer("dfire", self.rec_pdb, self.lig_pdb, **self.kwargs[c]) for c in "AB"}
        model = self.cpu["A"].model(0)
        assert np.array_equal(model["coordinates"], self.rec_xyz) and np.array_equal(self.cpu["A"].model(1)["coordinates"], self.lig_xyz)
        assert np.array_equal(self.cpu["B"].model(0)["restraint_atoms"], [0]) and np.array_equal(self.cpu["B"].model(1)["restraint_atoms"], [0])
        self.rec_types = model["dfire_types"]
        self.frames = pkg.dfire_route_frames(self.rec_xyz, self.lig_xyz, anm=self.anm, rec_types=self.rec_types)
        lo, hi, self.target_subtile, self.rec_order = subtile_boxes(pkg, model)
        self.sub_half = float(np.max(0.5 * (hi - lo)[self.target_subtile]))
        u = np.abs(rng.normal(size=3)) + 0.05
        self.u = u / np.linalg.norm(u)
        steps = pkg.dfire_bin_lut()
        self.nominal = [float(np.sqrt(steps[1][s])) for s in range(1, 21)] + [float(np.sqrt(steps[2])), 15.0]
        self.rotations = [np.array([1.0, 0.0, 0.0, 0.0])]
        for norm in (1.0, 1.7):
            for _ in range(200):
                q = rng.normal(size=4)
                q *= norm / np.linalg.norm(q)
                if self._clear(q) > CLEAR + 1.0:
                    break
            else:
                raise AssertionError("%s: no rotation keeps the anchors away" % name)
            self.rotations.append(q)
        self.poses, self.rho, self.energy, self.count, self.stats, self.special, self.brackets = {}, {}, {}, {}, {}, {}, {}
        for batch in self.batches:
            self._build(batch)

    # -- ANM
    @staticmethod
    def _modes(rng, n):
        m = rng.uniform(-0.02, 0.02, (3, n, 3))
        m[:, 0, :] = 0.0
        m[0, 0, 0], m[1, 0, 1], m[2, 0, 2] = 1.0, 0.5, 0.5
        return m

    def _tail(self, batch):
        return np.zeros(0) if not self.anm else np.concatenate([np.array(a, dtype=np.float64) for a in ANM_AMPS[batch]])

    def _shifts(self, batch):
        """How far the pose's amplitudes move every receptor / ligand atom (n, 3)."""
        if not self.anm:
            return np.zeros_like(self.rec_xyz), np.zeros_like(self.lig_xyz)
        a_rec, a_lig = (np.array(a) for a in ANM_AMPS[batch])
        return np.tensordot(a_rec, self.rec_modes, 1), np.tensordot(a_lig, self.lig_modes, 1)

    # -- poses
    def pose(self, q, rho, batch="rigid"):
        d_rec, d_lig = self._shifts(batch)
        t = (self.rec_xyz[0] + d_rec[0]) + rho * self.u - self.orc.q_rotate(q, self.lig_xyz[0]) - d_lig[0]
        return np.concatenate([t, q, self._tail(batch)])

    def _clear(self, q):
        """The smallest distance of any pair but the target pair over the ladder's whole range of rho (f64, both ends and the
        middle: a pair's distance is convex in rho) and over the batches."""
        worst = np.inf
        for batch in self.batches:
            d_rec, d_lig = self._shifts(batch)
            rec = self.rec_xyz + d_rec
            for rho in (0.0, 4.0, 8.0, 12.0, 16.0):
                row = self.pose(q, rho, batch)
                lig = self.lig_xyz @ _rotation(q).T + row[:3] + d_lig
                d = np.linalg.norm(lig[:, None, :] - rec[None, :, :], axis=-1)
                d[0, 0] = np.inf
                worst = min(worst, d.min())
        return worst

    def _answer(self, kind, q, rho, batch):
        row = self.pose(q, rho, batch)
        if kind == "cutoff":
            return self.cpu["A"].energy_ex_row(row)[1][5]
        return self.cpu["B" if kind == "interface" else "A"].energy_row(row)

    def _bisect(self, kind, q, nominal, batch):
        """(rho0, rho1): adjacent doubles, the oracle's answer at rho0 is the one at nominal - BRACKET, at rho1 it is another."""
        lo, hi = np.float64(nominal - BRACKET), np.float64(nominal + BRACKET)
        a_lo, a_hi = self._answer(kind, q, lo, batch), self._answer(kind, q, hi, batch)
        if a_lo == a_hi:
            raise AssertionError("%s %s at %.3f: the oracle answers %r on both ends of the bracket" % (self.name, kind, nominal, a_lo))
        lo_b, hi_b = int(lo.view(np.int64)), int(hi.view(np.int64))
        while hi_b - lo_b > 1:
            mid = (lo_b + hi_b) // 2
            if self._answer(kind, q, np.int64(mid).view(np.float64), batch) == a_lo:
                lo_b = mid
            else:
                hi_b = mid
        return float(np.int64(lo_b).view(np.float64)), float(np.int64(hi_b).view(np.float64))

    def _build(self, batch):
        names = edge_names()
        rows, rhos, brackets = [], [], []
        for q in self.rotations:
            for e, name in enumerate(names):
                kind = name if name in ("interface", "cutoff") else "step"
                rho0, rho1 = self._bisect(kind, q, self.nominal[e], batch)
                ladder = [rho0 - 2.0 ** -k for k in RUNG_KS] + [rho0, rho1] + [rho1 + 2.0 ** -k for k in reversed(RUNG_KS)]
                assert all(a < b for a, b in zip(ladder, ladder[1:])), (self.name, name)
                brackets.append((rho0, rho1))
                rhos.extend(ladder)
                rows.extend(self.pose(q, rho, batch) for rho in ladder)
        poses = np.ascontiguousarray(np.array(rows))
        self.poses[batch], self.rho[batch], self.brackets[batch] = poses, np.array(rhos), np.array(brackets)
        for c in "AB":
            ex = [self.cpu[c].energy_ex_row(p) for p in poses]
            self.energy[batch, c] = np.array([e for e, _ in ex])
            self.stats[batch, c] = np.array([s for _, s in ex])
            self.count[batch, c] = self.stats[batch, c][:, 5].astype(np.int64)
        # the one pose of a step-20 / cutoff ladder that sits at d2 == 225.0 exactly, if a double rho hits it: bin "20"
        a = self.energy[batch, "A"]
        self.special[batch] = (self.count[batch, "A"] == 1) & (np.abs(a - (4.7 - 0.0157 * 1.0)) < 1e-12) & (self.rho[batch] > 14.0)
        for arr in list(self.poses.values()) + list(self.rho.values()) + list(self.energy.values()) + list(self.count.values()):
            arr.setflags(write=False)

    def index(self, rotation, edge, rung):
        return (rotation * 22 + edge) * N_RUNGS + rung

    def label(self, i):
        r, rest = divmod(int(i), 22 * N_RUNGS)
        e, rung = divmod(rest, N_RUNGS)
        k = len(RUNG_KS)
        what = "rho0" if rung == k else "rho1" if rung == k + 1 else "rho0 - 2^-%d" % RUNG_KS[rung] if rung < k else "rho1 + 2^-%d" % RUNG_KS[2 * k + 1 - rung]
        return "%s rotation %d edge %s rung %s" % (self.name, r, edge_names()[e], what)

    def d2_target(self, batch="rigid"):
        """The target pair's squared distance per pose, in f64 with the oracle's rotation (src/qt.rs) and operation order."""
        poses = self.poses[batch]
        d_rec, d_lig = self._shifts(batch)
        out = np.empty(len(poses))
        per = 22 * N_RUNGS
        for r, q in enumerate(self.rotations):
            rot = self.orc.q_rotate(q, self.lig_xyz[0])
            lig = rot[None, :] + poses[r * per:(r + 1) * per, :3]
            for k in range(3 if self.anm else 0):
                lig = lig + self.lig_modes[k, 0][None, :] * ANM_AMPS[batch][1][k]
            rec = self.rec_xyz[0].copy()
            for k in range(3 if self.anm else 0):
                rec = rec + self.rec_modes[k, 0] * ANM_AMPS[batch][0][k]
            d = rec[None, :] - lig
            out[r * per:(r + 1) * per] = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        return out

    def cells_from_a_step(self, pkg, batch="rigid"):
        """Per pose: the distance of 64 d2 from the nearest bin step or the cutoff, in LUT cells of the block-major route."""
        steps = 64.0 * pkg.dfire_bin_lut()[1][1:]
        return np.abs(64.0 * self.d2_target(batch)[:, None] - steps[None, :]).min(1)


_CACHE = {}


def geometry(pkg, orc, table, directory, name):
    if name not in _CACHE:
        _CACHE[name] = Geometry(pkg, orc, table, directory, name)
    return _CACHE[name]


# ---- what the builder promises (asserted by the CPU test for every geometry) ------------------------------------------------

def check_edges(g):
    """Every edge realised by the oracle alone, nothing left out: the answers on the two sides differ by exactly the expected
    amount and are constant along each side's rungs; the target pair is the only pair in range."""
    k = len(RUNG_KS)
    names = edge_names()
    for batch in g.batches:
        eA, eB, cnt, stB, special = g.energy[batch, "A"], g.energy[batch, "B"], g.count[batch, "A"], g.stats[batch, "B"], g.special[batch]
        assert np.array_equal(cnt, g.count[batch, "B"])
        assert np.all((cnt == 0) | (cnt == 1)), "an anchor pair inside the cutoff"
        assert special.sum() <= 2 * len(g.rotations)
        for r in range(len(g.rotations)):
            for e, name in enumerate(names):
                i = g.index(r, e, 0)
                below, above = slice(i, i + k + 1), slice(i + k + 1, i + N_RUNGS)
                where = g.label(i + k)
                sp = special[i:i + N_RUNGS]
                assert sp.sum() <= 1 and (not sp.any() or (name in ("step20", "cutoff") and (sp[k] or sp[k + 1]))), where
                keep_lo, keep_hi = ~sp[:k + 1], ~sp[k + 1:]
                for arr in (eA, eB, cnt):
                    lo, hi = arr[below][keep_lo], arr[above][keep_hi]
                    assert np.all(lo == lo[0]) and np.all(hi == hi[-1]), (where, "not constant on a side")
                lo_A, hi_A, lo_B, hi_B = eA[i], eA[i + N_RUNGS - 1], eB[i], eB[i + N_RUNGS - 1]
                if name == "cutoff" or name == "step20":
                    assert cnt[i] == 1 and cnt[i + N_RUNGS - 1] == 0, where
                    assert cnt[i + k] == 1 and (cnt[i + k + 1] == 0 or sp[k + 1]), where          # one pair leaves between rho0 and rho1
                    assert abs(lo_A - (4.7 - 0.0157 * 20.0)) < 1e-12 and hi_A == 4.7 and lo_B == 4.7 and hi_B == 4.7, where
                    if name == "cutoff":
                        assert cnt[i + k + 1] == 0, where
                    else:
                        assert eA[i + k] == lo_A and eA[i + k + 1] != lo_A, where
                elif name == "interface":
                    assert cnt[i] == 1 and cnt[i + N_RUNGS - 1] == 1 and lo_A == hi_A, where
                    score = 4.7 - 0.0157 * 2.0
                    assert abs(hi_B - score) < 1e-12 and abs(lo_B - 3.0 * score) < 1e-12, where
                    assert np.all(stB[below][:, 2:4] == 1.0) and np.all(stB[above][:, 2:4] == 0.0), where
                    assert np.all(stB[below][:, 6:8] == 1.0) and np.all(stB[above][:, 6:8] == 0.0), where
                else:
                    s = e + 1   # bin s - 1 below, bin s above: the staircase grows by 1.0
                    assert cnt[i] == 1 and cnt[i + N_RUNGS - 1] == 1, where
                    assert abs(lo_A - (4.7 - 0.0157 * s)) < 1e-12 and abs((hi_A - lo_A) + 0.0157 * 1.0) < 1e-12, where
                    factor = 3.0 if s <= 1 else 1.0   # complex B: steps 1 and 2 lie on either side of the interface distance
                    want_hi = 0.0 if s == 19 else s + 1.0   # (its last bin is zero)
                    assert abs(lo_B - factor * (4.7 - 0.0157 * s)) < 1e-11 and abs(hi_B - factor * (4.7 - 0.0157 * want_hi)) < 1e-11, where
        for q in g.rotations:
            assert g._clear(q) > CLEAR, (g.name, "an anchor within %.1f A" % CLEAR)


# ---- the replay of the block-major f32 arithmetic (rigid form) -----------------------------------------------------------------

def fma32(a, b, c):
    """fl32(a * b + c) through f64 (module docstring)."""
    return (np.asarray(a, dtype=F32).astype(np.float64) * np.asarray(b, dtype=F32).astype(np.float64) + np.asarray(c, dtype=F32).astype(np.float64)).astype(F32)


def replay(pkg, g):
    """The target pair of every rigid pose of `g` as the block-major route computes it: dict(E (f32), truth = seed - 64 d2 in
    f64, err = |E - truth| in cells, eps = ld_dfire_bm_lut's for the frame (no subtile wider than the bound assumes), ratio =
    err / eps, eps_scorer = the bound with the receptor's own subtiles in it, code = that LUT's answer for floor(E) -- a LUT
    built for a larger eps flags more cells and answers the others alike --, operands: the magnitudes)."""
    assert not g.anm
    f = g.frames_compact["bm"]
    codes, eps = pkg.dfire_bm_lut(f["ubound"], f["lig_extent"])
    assert eps == f["eps"] and f["ubound"] == g.frames["bm"]["ubound"]
    c = f["centre"]
    rec = (8.0 * (g.rec_xyz - c[None, :])).astype(F32)                         # frame_coord: (float)(kappa (x - c))
    slots = g.rec_order[g.target_subtile * 8:g.target_subtile * 8 + 8]
    members = rec[slots[slots != 0xFFFFFFFF].astype(np.int64)]
    lo, hi = members.min(0), members.max(0)
    w, big = F32(2.0 ** -22), F32(3.0e38)
    lo, hi = fma32(-w, np.minimum(np.abs(lo), big), lo), fma32(w, np.minimum(np.abs(hi), big), hi)   # box_widen
    cb = F32(0.5) * (lo + hi)
    s = rec[0] - cb                                                              # bm_rec_ops
    seed = F32(SEED_CELL)
    Rs = fma32(-s[0], s[0], fma32(-s[1], s[1], fma32(-s[2], s[2], seed)))
    R2 = s * F32(2.0)
    poses = g.poses["rigid"]
    t, qw, qx, qy, qz = poses[:, :3], poses[:, 3], poses[:, 4], poses[:, 5], poses[:, 6]
    k = 8.0 / (qw * qw + qx * qx + qy * qy + qz * qz)                           # dfire_bm_pose
    M = [[k * (qw * qw + qx * qx - qy * qy - qz * qz), k * 2.0 * (qx * qy - qw * qz), k * 2.0 * (qx * qz + qw * qy)],
         [k * 2.0 * (qx * qy + qw * qz), k * (qw * qw - qx * qx + qy * qy - qz * qz), k * 2.0 * (qy * qz - qw * qx)],
         [k * 2.0 * (qx * qz - qw * qy), k * 2.0 * (qy * qz + qw * qx), k * (qw * qw - qx * qx - qy * qy + qz * qz)]]
    T = (8.0 * (t - c[None, :])).astype(F32)
    x = g.lig_xyz[0].astype(F32)                                                 # bm_lig_local
    L = []
    for a in range(3):
        tc = T[:, a] - cb[a]                                                     # the batch: translation - c, then bm_apply's three fmas
        L.append(fma32(M[a][0].astype(F32), x[0], fma32(M[a][1].astype(F32), x[1], fma32(M[a][2].astype(F32), x[2], tc))))
    l2 = fma32(L[0], L[0], fma32(L[1], L[1], L[2] * L[2]))
    E = Rs - l2                                                                  # bm_cell
    E = fma32(R2[2], L[2], E)
    E = fma32(R2[1], L[1], E)
    E = fma32(R2[0], L[0], E)
    truth = SEED_CELL - 64.0 * g.d2_target()
    err = np.abs(E.astype(np.float64) - truth)
    cell = np.where(E >= 0, np.minimum(E, F32(4.0e9)), F32(0.0)).astype(np.int64)   # v_cvt_u32_f32: negative -> 0
    in_lut = cell < len(codes)
    code = np.where(in_lut, codes[np.minimum(cell, len(codes) - 1)], -1)
    return dict(E=E, truth=truth, err=err, eps=eps, ratio=err / eps, eps_scorer=g.frames["bm"]["eps"], code=code, cell=cell,
                operands=dict(r_minus_c=float(np.abs(s).max()), l_minus_c=float(max(np.abs(v).max() for v in L)), l2=float(l2.max()), Rs=float(abs(Rs))))


def decisions_of(g, code, batch="rigid"):
    """Which poses the LUT codes `code` decide WRONGLY for the target pair, against the oracle (complex A): a code that is not
    flagged must be the miss code where the oracle counts no pair, and 8 x the oracle's bin where it counts one."""
    cnt, e = g.count[batch, "A"], g.energy[batch, "A"]
    bins = np.rint((4.7 - e) / 0.0157).astype(np.int64) - 1          # the staircase: v = bin + 1
    want = np.where(cnt == 1, 8 * bins, MISS)
    want = np.where(g.special[batch], FLAGGED, want)                   # d2 == 225.0 exactly: only the exact path reads bin "20"
    return (code != FLAGGED) & (code != want)
