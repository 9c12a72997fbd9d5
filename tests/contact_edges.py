"""Residue contacts ON their threshold at every pruning level: synthetic complexes whose posed thousandths are integers by
construction, the poses that put one chosen atom pair at d^2 == C^2 (in) or at the smallest reachable sum of three squares above
it (out) wherever complex_contacts (kernels/cluster.hip) and complex_pair_sets (kernels/fcc.hip) decide -- the receptor residue's
box against the whole ligand's, against a group of kResGroup ligand residues, against one ligand residue, and the 8 x 8 atom walk
with in_contact (kernels/complex_pose.hpp) -- and the exact oracle: all atom pairs on int64, no boxes, no clamps.
Shared by tests/test_contact_edges_cpu.py (a replay of the walk proves every case is what it says) and
tests/test_gpu_contact_edges.py (both kernels against the oracle, word for word).  No test functions here; numpy and the
standard library.

Complexes (`Shape`).  A LINE shape has its receptor residues along x and its ligand residues along y at one pitch, the ligand
500 A above the receptor at rest (rows of ROW ligand residues, a row 1000 A above the one before, when the ligand is longer than
the PDB columns allow).  A residue is one atom named CA, but for a few of 8, 9 and 17 atoms spread by 0.1 A steps along z and one
a side of three atoms 1 A apart (the partner between two of them is what no box sees: level d).  Every coordinate is a whole
number of thousandths.  A pose is a half turn (or none) and a whole-thousandth translation that puts ligand
atom (L, ib) at receptor atom (R, ia) + v: every other residue pair is then more than 2 C apart (the pitch is above 3 C), and
with v = (a, b, 0 or 1) the chosen pair is the only one of its two residues at its distance (the neighbours along z are 0.1 A
off), given that two residues of several atoms meet end to end.  The FLEX shape adds one receptor mode that moves residue r by
(r % 5, 2 (r % 3), 1000 + 7 r % 11) thousandths a unit of amplitude; the BIG shape has 1100 ligand residues, more boxes than the
kernels keep in LDS.  The MOTIF shape holds copies of six residues in contact as the skip of complex_contacts needs them (below).

The out twins of the levels a to c.  The reading taken: the residues of these cases have one atom each (L = 516 has nine, atom 0
deciding), the in twin is v = (0, +-C, 0) and the out twin v = (0, +-(C + 1), 0) -- one box gap a thousandth beyond equality, the
other two axes' projections at 0, inside C -- so nothing but the box arithmetic on y separates the twins.  There is no second
atom pair inside C on the other axes: a box that wrongly accepts an out twin cannot change the result (the atoms still say
out), so the sensitivity to the box test lies with the in twins, which a `<` for `<=` at their level rejects.
"""
import collections
import functools
import itertools
import math
import os

import numpy as np

RES_GROUP = 8             # kResGroup (kernels/cluster.hpp)
TILE = 8                  # atoms a side of one step of the atom walk
WAVES = 8                 # kContactThreads / 64 == kPairThreads / 64
SCAN_CHUNK = 512          # kPairThreads: words of the pair bitmap a step of the key scan
MAX_BOX_LDS_BYTES = 40 << 10
COORD_BOUND = 10 ** 9     # thousandths

ROTATIONS = {"I": ((1.0, 0.0, 0.0, 0.0), (1, 1, 1)), "X": ((0.0, 1.0, 0.0, 0.0), (1, -1, -1)),
             "Y": ((0.0, 0.0, 1.0, 0.0), (-1, 1, -1)), "Z": ((0.0, 0.0, 0.0, 1.0), (-1, -1, 1))}

LIG_Z0 = 500000
ROW = 517
ROW_Z = 1000000
ATOM_STEP = 100
WIDE_STEP = 1000


# ---- shapes -------------------------------------------------------------------------------------------------------------------

class Shape:
    """rec, lig: int64 (atoms, 3) thousandths at rest; rec_of, lig_of: the residue of every atom; mode: int64 (receptor atoms, 3)
    thousandths a unit of amplitude, or None."""

    def __init__(self, name, rec, rec_of, lig, lig_of, mode=None):
        self.name = name
        self.rec, self.lig = np.asarray(rec, dtype=np.int64), np.asarray(lig, dtype=np.int64)
        self.rec_of, self.lig_of = np.asarray(rec_of, dtype=np.int64), np.asarray(lig_of, dtype=np.int64)
        self.mode = None if mode is None else np.asarray(mode, dtype=np.int64)
        self.n_rec_res, self.n_lig_res = int(self.rec_of[-1]) + 1, int(self.lig_of[-1]) + 1
        self.rec_start = np.searchsorted(self.rec_of, np.arange(self.n_rec_res + 1))
        self.lig_start = np.searchsorted(self.lig_of, np.arange(self.n_lig_res + 1))
        self.n_lig_grp = (self.n_lig_res + RES_GROUP - 1) // RES_GROUP
        self.lig_words = (self.n_lig_res + 31) // 32

    @property
    def n_boxes(self):
        return self.n_rec_res + self.n_lig_res + self.n_lig_grp

    @property
    def boxes_in_lds(self):
        return self.n_boxes * 24 <= MAX_BOX_LDS_BYTES

    @property
    def pose_len(self):
        return 7 + (self.mode is not None)

    def size(self, side, r):
        start = self.rec_start if side == 0 else self.lig_start
        return int(start[r + 1] - start[r])

    def single(self, side, r):
        """The first residue from r on, of the side, with one atom."""
        n = self.n_rec_res if side == 0 else self.n_lig_res
        while self.size(side, r % n) != 1:
            r += 1
        return r % n


def residue_atoms(centres, sizes):
    xyz, of = [], []
    for r, c in enumerate(centres):
        n, step = sizes.get(r, (1, 0))
        for k in range(n):
            xyz.append((c[0], c[1], c[2] + step * k))
            of.append(r)
    return xyz, of


def line_shape(name, n_rec, n_lig, pitch, rec_sizes, lig_sizes, flex=False):
    rec, rec_of = residue_atoms([(pitch * i, 0, 0) for i in range(n_rec)], rec_sizes)
    lig, lig_of = residue_atoms([(0, pitch * (j % ROW), LIG_Z0 + ROW_Z * (j // ROW)) for j in range(n_lig)], lig_sizes)
    mode = [(r % 5, 2 * (r % 3), 1000 + 7 * r % 11) for r in rec_of] if flex else None
    return Shape(name, rec, rec_of, lig, lig_of, mode)


# residue -> (atoms, their step along z): 8, 9 and 17 atoms 0.1 A apart, and three atoms 1 A apart
REC_SIZES = {100: (8, ATOM_STEP), 101: (9, ATOM_STEP), 102: (17, ATOM_STEP), 103: (3, WIDE_STEP), 519: (9, ATOM_STEP)}
LIG_SIZES = {200: (8, ATOM_STEP), 201: (9, ATOM_STEP), 202: (17, ATOM_STEP), 203: (3, WIDE_STEP), 516: (9, ATOM_STEP)}

# Six residues: R1 touches L1, L2 and L3, R2 touches L2, R3 touches L1; L3 touches nothing but R1, R3 nothing but L1.  Every
# touching pair is 4 A apart, every other pair of the six more than 8.9 A.  Thousandths, relative to the copy's place.
MOTIF_REC = {"R1": (4000, 0, 0), "R2": (-4000, 0, 0), "R3": (8000, -4000, 0)}
MOTIF_LIG = {"L1": (8000, 0, 0), "L2": (0, 0, 0), "L3": (4000, 4000, 0)}
MOTIF_PAIRS = (("R1", "L1"), ("R1", "L2"), ("R1", "L3"), ("R2", "L2"), ("R3", "L1"))
MOTIF_C = 4000
MOTIF_N_REC, MOTIF_N_LIG = 72, 264          # 72 x 9 words of pair bitmap: two scan chunks
# (R1, R2, R3), (L1, L2, L3) of every copy.  Receptor residue r is walked by wave r % 8, a wave's residues in ascending order,
# a residue's ligand partners in ascending order.
MOTIFS = (((0, 8, 16), (0, 1, 2)),          # one wave, one group, everything in order
          ((24, 1, 9), (12, 10, 11)),       # R3 = 9 in another wave than R1; L3 between L2 and L1
          ((33, 17, 25), (40, 31, 32)),     # R1 behind R2 and R3 in their wave; L2 in the group before L1's
          ((2, 3, 4), (50, 60, 70)),        # three waves, three groups
          ((56, 57, 64), (255, 256, 257)),  # words 511 and 512 of the bitmap: either side of a scan chunk's end
          ((71, 70, 63), (263, 100, 262)))  # the last residues of both sides, L3 in the partial last group


def motif_shape():
    rec_at, lig_at = {}, {}
    for k, (rs, ls) in enumerate(MOTIFS):
        place = np.array([200000 * k, 0, 0])
        for name, r in zip(("R1", "R2", "R3"), rs):
            assert r not in rec_at
            rec_at[r] = place + MOTIF_REC[name]
        for name, l in zip(("L1", "L2", "L3"), ls):
            assert l not in lig_at
            lig_at[l] = place + MOTIF_LIG[name]
    rec = [rec_at.get(r, (16000 * r, 100000, 500000)) for r in range(MOTIF_N_REC)]
    lig = [lig_at.get(l, (16000 * l, -100000, -500000)) for l in range(MOTIF_N_LIG)]
    return Shape("motif", rec, np.arange(MOTIF_N_REC), lig, np.arange(MOTIF_N_LIG))


@functools.lru_cache(maxsize=None)
def shape(name):
    if name == "base":
        return line_shape("base", 520, 517, 16000, REC_SIZES, LIG_SIZES)
    if name == "flex":
        return line_shape("flex", 520, 517, 16000, REC_SIZES, LIG_SIZES, flex=True)
    if name == "big":
        return line_shape("big", 520, 1100, 16000, REC_SIZES, LIG_SIZES)
    if name == "small":
        return line_shape("small", 20, 19, 120000, {5: (17, ATOM_STEP)}, {6: (9, ATOM_STEP), 18: (9, ATOM_STEP)})
    assert name == "motif"
    return motif_shape()


SHAPES = ("base", "flex", "big", "small", "motif")


def pdb_line(serial, name, resname, chain, seq, xyz):
    return "ATOM  %5d  %-3s %3s %1s%4d    %8.3f%8.3f%8.3f  1.00  0.00           C\n" % (
        serial, name, resname, chain, seq, xyz[0] / 1000.0, xyz[1] / 1000.0, xyz[2] / 1000.0)


def write_complex(sh, directory):
    """The two PDB files in `directory` and the receptor's mode array in A: (rec_pdb, lig_pdb, rec_modes or None)."""
    paths = []
    for tag, chain, resname, xyz, of in (("rec", "A", "GLY", sh.rec, sh.rec_of), ("lig", "B", "ALA", sh.lig, sh.lig_of)):
        assert xyz.min() >= -999999 and xyz.max() <= 9999999          # the PDB columns
        path = os.path.join(directory, "%s_%s.pdb" % (sh.name, tag))
        first = np.searchsorted(of, of)
        with open(path, "w") as f:
            for a in range(len(xyz)):
                k = a - first[a]
                f.write(pdb_line(a + 1, "CA" if k == 0 else "C%d" % k, resname, chain, of[a] + 1, xyz[a]))
        paths.append(path)
    modes = None if sh.mode is None else (sh.mode / 1000.0)[None]
    return paths[0], paths[1], modes


def make_complex(pkg, sh, directory):
    rec, lig, modes = write_complex(sh, directory)
    return pkg.Complex(rec, lig, modes, 0 if modes is None else 1)


# ---- poses ----------------------------------------------------------------------------------------------------------------------

# t: the translation in thousandths; rot: a key of ROTATIONS; amp: the receptor mode's amplitude (an integer);
# pair: (R, ia, L, ib), the atom pair the pose is built around, or None; kind: "in", "out" or None; S: the d^2 meant for the pair;
# tags: what the builder means the pose to cover.
Pose = collections.namedtuple("Pose", "t rot amp pair kind S tags")
Case = collections.namedtuple("Case", "name shape C poses")


def posed(sh, pose):
    """(receptor atoms, ligand atoms) of the pose, int64 thousandths, in integer arithmetic."""
    rec = sh.rec if not pose.amp else sh.rec + pose.amp * sh.mode
    return rec, sh.lig * np.array(ROTATIONS[pose.rot][1], dtype=np.int64) + np.array(pose.t, dtype=np.int64)


def place(sh, R, ia, L, ib, v, rot="I", amp=0, kind=None, tags=()):
    """The pose that puts ligand atom ib of residue L at receptor atom ia of residue R + v."""
    assert ia < sh.size(0, R) and ib < sh.size(1, L)
    ra, la = int(sh.rec_start[R]) + ia, int(sh.lig_start[L]) + ib
    if sh.mode is None:
        amp = 0
    at = sh.rec[ra] + (amp * sh.mode[ra] if amp else 0)
    t = at + np.array(v, dtype=np.int64) - np.array(ROTATIONS[rot][1], dtype=np.int64) * sh.lig[la]
    return Pose(tuple(int(x) for x in t), rot, amp, (R, ia, L, ib), kind, sum(int(x) ** 2 for x in v), tuple(tags))


def rows(sh, poses):
    """The pose rows of the calls: translation in A, quaternion, the amplitude where the receptor flexes."""
    out = np.zeros((len(poses), sh.pose_len))
    for i, p in enumerate(poses):
        out[i, :3] = [x / 1000.0 for x in p.t]
        out[i, 3:7] = ROTATIONS[p.rot][0]
        if sh.mode is not None:
            out[i, 7] = float(p.amp)
    return out


# ---- sums of squares ----------------------------------------------------------------------------------------------------------

def two_squares(N, least=0):
    """(a, b), a >= b >= least, a^2 + b^2 == N, or None."""
    a = math.isqrt(N)
    while 2 * a * a >= N:
        b = math.isqrt(N - a * a)
        if b * b == N - a * a and b >= least:
            return a, b
        a -= 1
    return None


def three_nonzero(S):
    """(a, b, c), all at least 1, with a^2 + b^2 + c^2 == S, c as small as it gets."""
    for c in range(1, math.isqrt(S // 3) + 1):
        ab = two_squares(S - c * c, least=c)
        if ab:
            return ab + (c,)
    raise AssertionError(S)


def small_z(S, least, exact):
    """((a, b, c), S'), least <= c < WIDE_STEP / 2: the first S' >= S that has one (S itself with `exact`)."""
    while True:
        for c in range(least, WIDE_STEP // 2):
            ab = two_squares(S - c * c)
            if ab:
                return ab + (c,), S
        assert not exact, S
        S += 1


def arrangements(triple):
    """Every order and sign of the triple, each vector once."""
    return sorted({tuple(s * x for s, x in zip(signs, perm)) for perm in itertools.permutations(triple)
                   for signs in itertools.product((1, -1), repeat=3)})


def threshold_vectors(C):
    """[(kind, axes, vector)]: d^2 == C^2 on one, two and three axes, and C^2 + 1 -- the smallest sum of three squares above
    -- next to each; C + 1 along one axis too, the nearest out that one axis reaches."""
    assert C % 5 == 0 and C >= 25
    on = {1: (C, 0, 0), 2: (3 * C // 5, 4 * C // 5, 0), 3: (12 * C // 25, 16 * C // 25, 3 * C // 5)}
    off = {1: (C, 1, 0), 2: (3 * C // 5, 4 * C // 5, 1), 3: three_nonzero(C * C + 1)}
    out = []
    for axes in (1, 2, 3):
        assert sum(x * x for x in on[axes]) == C * C and sum(x * x for x in off[axes]) == C * C + 1
        out += [("in", axes, v) for v in arrangements(on[axes])] + [("out", axes, v) for v in arrangements(off[axes])]
    return out + [("out", 1, v) for v in arrangements((C + 1, 0, 0))]


# ---- the cases ----------------------------------------------------------------------------------------------------------------

AMPS = (0, 1, -3, 7, 50, -50, 12)
WALK_R = (0, 7, 8, 511, 512, 513, 519)
WALK_L = (0, 7, 8, 511, 512, 516)
WALK_BOTH = ((0, 0), (512, 512), (513, 511), (519, 516))
LEVEL_R = 250
# (level, L, where L stands in what the level's box holds: "first" or "last"; None: anywhere)
LEVEL_L = (("a", 0, "first"), ("a", 516, "last"), ("b", 8, "first"), ("b", 15, "last"), ("b", 504, "first"), ("b", 511, "last"),
           ("b", 512, "first"), ("c", 10, None), ("c", 514, None))
REC_LADDER = [(R, ia) for R, at in ((100, (0, 7)), (101, (0, 7, 8)), (102, (0, 7, 8, 16))) for ia in at]
LIG_LADDER = [(L, ib) for L, at in ((200, (0, 7)), (201, (0, 7, 8)), (202, (0, 7, 8, 16))) for ib in at]
# two residues of several atoms meet end to end: (R, ia, L, ib, rotation); under X and Y the ligand's atoms descend along z
ATOM_PAIRINGS = ((102, 16, 202, 0, "I"), (102, 0, 202, 16, "I"), (102, 16, 202, 16, "X"), (102, 0, 202, 0, "X"),
                 (101, 8, 201, 8, "Y"), (100, 7, 200, 0, "I"), (519, 8, 516, 8, "X"))


def twins(sh, R, ia, L, ib, v_in, v_out, rot, amps, tags):
    return [place(sh, R, ia, L, ib, v_in, rot, next(amps), "in", tags), place(sh, R, ia, L, ib, v_out, rot, next(amps), "out", tags)]


def chunk_words(sh):
    """Words of the pair bitmap at either side of a scan chunk's end, and the last one: [(word, "first" or "last")]."""
    words = sh.n_rec_res * sh.lig_words
    assert words > 2 * SCAN_CHUNK
    return [(SCAN_CHUNK - 1, "last"), (SCAN_CHUNK, "first"), (2 * SCAN_CHUNK - 1, "last"), (2 * SCAN_CHUNK, "first"),
            (words - 1, "last")]


@functools.lru_cache(maxsize=None)
def edge_case(shape_name, C=5000):
    """What base, flex and big share: the level at which the decision falls, the places in the walk, the deciding atom, the
    scan chunks of the pair bitmap and the far poses.  The poses of flex take the amplitudes of AMPS in turn."""
    sh = shape(shape_name)
    amps = itertools.cycle(AMPS)
    v_in, v_out = (3 * C // 5, 4 * C // 5, 0), (3 * C // 5, 4 * C // 5, 1)
    poses = []
    # the level: a vector along y, the ligand's residues on the far side of L where L is first or last
    for rot in ("I", "X"):
        sy = ROTATIONS[rot][1][1]
        for level, L, stands in LEVEL_L:
            side = -sy if stands == "last" else sy
            poses += twins(sh, LEVEL_R, 0, L, 0, (0, side * C, 0), (0, side * (C + 1), 0), rot, amps, ("level", level))
    d_in, _ = small_z(C * C, 1, True)
    d_out, _ = small_z(C * C + 1, 2, False)
    # d: the middle atom of three 1 A apart along z, the partner between it and the next: no box sees the z of the vector
    poses += twins(sh, 103, 1, 300, 0, d_in, d_out, "I", amps, ("level", "d"))
    poses += twins(sh, LEVEL_R, 0, 203, 1, d_in, d_out, "I", amps, ("level", "d"))
    poses += twins(sh, 103, 1, 300, 0, tuple(-x for x in d_in), tuple(-x for x in d_out), "Z", amps, ("level", "d"))
    # the places
    for R in WALK_R:
        poses += twins(sh, R, 0, 100, 0, v_in, v_out, "I", amps, ("walk", "R", R))
    for L in WALK_L:
        poses += twins(sh, LEVEL_R, 0, L, 0, v_in, v_out, "I", amps, ("walk", "L", L))
    for R, L in WALK_BOTH:
        rot = "X" if sh.size(0, R) > 1 and sh.size(1, L) > 1 else "I"
        poses += twins(sh, R, 0, L, 0, v_in, v_out, rot, amps, ("walk", "both", R, L))
    # the deciding atom
    # (the out twin's thousandth along z points into the residue of several atoms: its box hides it, so the atoms decide)
    for R, ia in REC_LADDER:
        inward = 1 if ia < sh.size(0, R) - 1 else -1
        poses += twins(sh, R, ia, 300, 0, v_in, v_out[:2] + (inward,), "I", amps, ("atom", "rec"))
    for L, ib in LIG_LADDER:
        inward = -1 if ib < sh.size(1, L) - 1 else 1
        poses += twins(sh, LEVEL_R, 0, L, ib, v_in, v_out[:2] + (inward,), "I", amps, ("atom", "lig"))
    for R, ia, L, ib, rot in ATOM_PAIRINGS:
        poses += twins(sh, R, ia, L, ib, v_in, v_out, rot, amps, ("atom", "both"))
    # the pair bitmap's scan chunks
    for word, where in chunk_words(sh):
        r, l = word // sh.lig_words, min(word % sh.lig_words * 32 + (31 if where == "last" else 0), sh.n_lig_res - 1)
        rot = "X" if sh.size(0, r) > 1 and sh.size(1, l) > 1 else "I"
        poses += twins(sh, r, 0, l, 0, v_in, v_out, rot, amps, ("chunk", where))
    # far: no key at all.  The ligand 990 000 A above the receptor; where the receptor flexes, 1.9e6 A between the two
    poses.append(Pose((0, 0, 990000000), "I", 0, None, None, None, ("far", "apart")))
    if sh.mode is not None:
        poses.append(Pose((0, 0, 950000000 - LIG_Z0), "Y", -949000, None, None, None, ("far", "1.9e6")))
    return Case("edges-%s-C%d" % (shape_name, C), shape_name, C, tuple(poses))


def scattered(sh, k):
    """Residues of one atom each, another pair for every k."""
    return sh.single(0, (37 * k + 5) % sh.n_rec_res), sh.single(1, (53 * k + 11) % sh.n_lig_res)


@functools.lru_cache(maxsize=None)
def vector_case(shape_name, C):
    """d^2 == C^2 and the sums just above on one, two and three axes, in every order and sign."""
    sh = shape(shape_name)
    poses = []
    for k, (kind, axes, v) in enumerate(threshold_vectors(C)):
        R, L = scattered(sh, k)
        poses.append(place(sh, R, 0, L, 0, v, "IXYZ"[k % 4], 0, kind, ("vector", axes)))
    return Case("vectors-%s-C%d" % (shape_name, C), shape_name, C, tuple(poses))


@functools.lru_cache(maxsize=None)
def thousandth_case():
    """Cutoff 0.001: (0, 0, 0) and (1, 0, 0) are in, (1, 1, 0) is out."""
    sh = shape("base")
    vectors = [("in", (0, 0, 0))] + [("in", v) for v in arrangements((1, 0, 0))]
    vectors += [("out", v) for v in arrangements((1, 1, 0)) + arrangements((1, 1, 1)) + arrangements((2, 0, 0))]
    poses = []
    for k, (kind, v) in enumerate(vectors):
        R, L = scattered(sh, k)
        poses.append(place(sh, R, 0, L, 0, v, "IXYZ"[k % 4], 0, kind, ("thousandth",)))
    return Case("thousandth", "base", 1, tuple(poses))


FAR = (32767, 32768, 40000)


@functools.lru_cache(maxsize=None)
def far_case(C):
    """Differences the 32-bit test must clamp, not wrap: 32767, 32768 and 40000 on one axis with the other two at 0; 65536 along z,
    whose square is 2^32; 40000 on all three, whose squares sum to 2^32 + 505 032 704.  All out."""
    sh = shape("small")
    vectors = [v for d in FAR for v in arrangements((d, 0, 0))] + arrangements((40000, 40000, 40000))[:2] + [(0, 0, 65536), (0, 0, -65536)]
    poses = []
    for k, v in enumerate(vectors):
        R, L = scattered(sh, k)
        poses.append(place(sh, R, 0, L, 0, v, "IXYZ"[k % 4], 0, "out", ("far", max(abs(x) for x in v))))
    return Case("far-C%d" % C, "small", C, tuple(poses))


@functools.lru_cache(maxsize=None)
def motif_case():
    """Every copy of the six residues at once: at rest every touching pair is MOTIF_C apart exactly; a thousandth along z and
    every one of them is at MOTIF_C^2 + 1; 50 A along y and nothing touches."""
    poses = (Pose((0, 0, 0), "I", 0, None, "in", None, ("motif",)), Pose((0, 0, 1), "I", 0, None, "out", None, ("motif",)),
             Pose((0, 0, -1), "I", 0, None, "out", None, ("motif",)), Pose((0, 50000, 0), "I", 0, None, None, None, ("far", "apart")))
    return Case("motif", "motif", MOTIF_C, poses)


def all_cases():
    for name in ("base", "flex", "big"):
        yield edge_case(name)
    yield vector_case("base", 5000)
    yield thousandth_case()
    yield vector_case("small", 30000)
    yield far_case(30000)
    yield far_case(5000)
    yield motif_case()


def case_named(name):
    return {c.name: c for c in all_cases()}[name]


CASE_NAMES = tuple(c.name for c in all_cases())


# ---- the oracle: all pairs on int64 -------------------------------------------------------------------------------------------

# rec, lig: bool per residue; keys: ascending int64 r * n_lig_res + l; near: (receptor atom, ligand atom, d^2) int64 rows of every
# atom pair within 2 C, by receptor atom, then ligand atom.
Expect = collections.namedtuple("Expect", "rec lig keys near")


def oracle(sh, pose, C):
    """A receptor and a ligand residue touch when some atom pair has dx^2 + dy^2 + dz^2 <= C^2."""
    rec, lig = posed(sh, pose)
    span = [int(max(rec[:, k].max() - lig[:, k].min(), lig[:, k].max() - rec[:, k].min())) for k in range(3)]
    assert sum(s * s for s in span) < 2 ** 63 and max(int(np.abs(rec).max()), int(np.abs(lig).max())) <= COORD_BOUND
    d2 = np.zeros((len(rec), len(lig)), dtype=np.int64)
    d = np.empty_like(d2)
    for k in range(3):
        np.subtract(rec[:, None, k], lig[None, :, k], out=d)
        np.multiply(d, d, out=d)
        d2 += d
    ra, la = np.nonzero(d2 <= 4 * C * C)
    near = np.stack([ra, la, d2[ra, la]], axis=1).astype(np.int64)
    touch = near[near[:, 2] <= C * C]
    rec_bits, lig_bits = np.zeros(sh.n_rec_res, dtype=bool), np.zeros(sh.n_lig_res, dtype=bool)
    rec_bits[sh.rec_of[touch[:, 0]]] = True
    lig_bits[sh.lig_of[touch[:, 1]]] = True
    keys = np.unique(sh.rec_of[touch[:, 0]] * sh.n_lig_res + sh.lig_of[touch[:, 1]])
    return Expect(rec_bits, lig_bits, keys.astype(np.int64), near)


@functools.lru_cache(maxsize=None)
def expected(case_name):
    """The oracle on every pose of the case, once: a tuple of Expect."""
    case = case_named(case_name)
    sh = shape(case.shape)
    return tuple(oracle(sh, p, case.C) for p in case.poses)


def expected_words(case_name):
    """-> (rec bool (n, receptor residues), lig bool (n, ligand residues), offsets (n + 1,), keys) of the case."""
    ex = expected(case_name)
    offsets = np.zeros(len(ex) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(e.keys) for e in ex])
    return (np.array([e.rec for e in ex]), np.array([e.lig for e in ex]), offsets,
            np.concatenate([e.keys for e in ex]) if len(ex) else np.zeros(0, dtype=np.int64))


def projection(sh, offsets, keys):
    """The residues the keys name: (bool (n, receptor residues), bool (n, ligand residues))."""
    n = len(offsets) - 1
    rec, lig = np.zeros((n, sh.n_rec_res), dtype=bool), np.zeros((n, sh.n_lig_res), dtype=bool)
    for i in range(n):
        k = np.asarray(keys[offsets[i]:offsets[i + 1]], dtype=np.int64)
        rec[i, k // sh.n_lig_res] = True
        lig[i, k % sh.n_lig_res] = True
    return rec, lig
