"""The clustering's RMSD test ON its threshold: an exact integer oracle of `round(rmsd, 4) <= cutoff`, synthetic complexes whose
posed thousandths are integers by construction, and the cases that put S -- the integer sum of squared differences of two poses'
printed thousandths -- at floor(s*) (in) and floor(s*) + 1 (out) wherever complex_bsas (kernels/cluster.hip), ranked_pick and
ranked_sweep (kernels/ranked.hip) decide it: within_cutoff, the bisected s_max and thousandths() of kernels/complex_pose.hpp.
Shared by tests/test_bsas_edges_cpu.py (the oracle against the tool's rule, and every case is what it says) and
tests/test_gpu_bsas_edges.py (both calls against the oracle, word for word).  No test functions here; numpy and the standard library.

The rule.  lgd_cluster_bsas.py joins a pose to a representative iff round(sqrt(S * 1e-6 / n), 4) <= cutoff, n the atoms measured.
round(x, 4) is m / 1e4 for the integer m nearest x * 1e4, and m / 1e4 <= cutoff iff m <= K, K the largest integer with
K / 1e4 <= cutoff (`threshold_K`).  m <= K iff sqrt(S * 1e2 / n) < K + 1/2 iff 400 S < n (2K + 1)^2: `within`.  Equality is a TIE
(`is_tie`): the exact rmsd * 1e4 is a half and the float path decides; a tie needs 16 | n and 25 | n (2K + 1)^2, no case of all_cases() is one,
and tests/test_bsas_edges_cpu.py holds that.  s* = n (2K + 1)^2 / 400; `s_floor` is floor(s*), the largest S within.

Complexes (`Spec`).  A side is n_bb residues of N, CA (every third ligand residue: P), C -- so backbone index != atom index -- on a
3.75 A lattice: every coordinate is a multiple of 0.125 A and prints exactly.  An empty side is a single N atom.  A MOVER is a
backbone atom with three normal modes that move only it, by 1.0 along x, y and z: an extent of d / 1000 displaces it by d thousandths.
Every pose has the identity rotation, under which the posing is (L + extents) + t on the ligand and R + extents on the receptor,
one rounding a term: `posed` restates it in numpy, `printed_thousandths` reads the decimal expansion of the double.

Order.  complex_bsas walks the receptor's backbone atoms, then the ligand's; ranked clustering walks the ligand's first and the
receptor's only when receptor modes exist, 32 atoms a granule in both.  The layouts of `where_case` put movers at backbone index
0, 31, 32, 63, 64 and the last of either order.
"""
import collections
import decimal
import functools
import math
import os

import numpy as np

INF = float("inf")
MEASURES = ("complex", "ligand")


# ---- the exact oracle ---------------------------------------------------------------------------------------------------------

def threshold_K(cutoff):
    """The largest integer K with K / 1e4 <= cutoff; None for a negative cutoff (nothing is within), inf for inf."""
    assert not math.isnan(cutoff)
    if cutoff < 0.0:
        return None
    if cutoff == INF:
        return INF
    assert cutoff * 1e4 < 2.0 ** 52
    K = int(math.floor(cutoff * 1e4))
    while (K + 1) / 1e4 <= cutoff:
        K += 1
    while K / 1e4 > cutoff:
        K -= 1
    return K


def within(S, n, cutoff):
    """round(sqrt(S * 1e-6 / n), 4) <= cutoff in integers (off a tie)."""
    K = threshold_K(cutoff)
    if K is None:
        return False
    if K == INF:
        return True
    return 400 * int(S) < int(n) * (2 * K + 1) ** 2


def is_tie(S, n, cutoff):
    K = threshold_K(cutoff)
    return K is not None and K != INF and 400 * int(S) == int(n) * (2 * K + 1) ** 2


def s_floor(n, cutoff):
    """floor(s*): the largest S within the (finite, non-negative) cutoff, unless s* is an integer (a tie)."""
    return int(n) * (2 * threshold_K(cutoff) + 1) ** 2 // 400


def printed_thousandths(x):
    """The integer c with "%.3f" % x == c / 1000, from the exact decimal expansion of the double, half-even."""
    d = decimal.Decimal(float(x)).quantize(decimal.Decimal("0.001"), rounding=decimal.ROUND_HALF_EVEN)
    return int(d.scaleb(3))


def thousandths_of(X):
    """printed_thousandths elementwise, int64 (each distinct double once)."""
    X = np.asarray(X, dtype=np.float64)
    values, inverse = np.unique(X.ravel(), return_inverse=True)
    ints = np.array([printed_thousandths(v) for v in values], dtype=np.int64)
    return ints[inverse].reshape(X.shape)


def sum_sq(a, b):
    """The sum of squared differences of two int64 rows, as a Python int."""
    return sum((int(u) - int(v)) ** 2 for u, v in zip(a, b))


def bsas(T, n_atoms, scoring, cutoff, trace=None):
    """Sequential BSAS over integer S: poses (rows of T, the thousandths of the measured atoms) by score descending, then index
    ascending; a pose joins the first representative, in creation order, that is `within`, else founds a cluster.  Returns
    (cluster_of, representatives, ties), ties counting the comparisons made that were `is_tie`.  `trace` collects every S compared."""
    T = np.asarray(T, dtype=np.int64)
    n = len(T)
    order = sorted(range(n), key=lambda i: (-float(scoring[i]), i))
    fast = T.size == 0 or T.shape[1] * (2 * int(np.abs(T).max())) ** 2 < 2 ** 63   # no int64 sum below can wrap
    reps, cluster_of, ties = [], [-1] * n, 0
    for i in order:
        if fast:
            d = T[reps] - T[i]
            sums = [int(s) for s in (d * d).sum(axis=1)]
        else:
            sums = [sum_sq(T[r], T[i]) for r in reps]
        for c, S in enumerate(sums):
            if trace is not None:
                trace.append(S)
            ties += is_tie(S, n_atoms, cutoff)
            if within(S, n_atoms, cutoff):
                cluster_of[i] = c
                break
        else:
            cluster_of[i] = len(reps)
            reps.append(i)
    return cluster_of, reps, ties


# ---- sums of squares ----------------------------------------------------------------------------------------------------------

def three_squares(S):
    """(a, b, c), a >= b >= c >= 0, with a^2 + b^2 + c^2 == S, a as large as it gets; None where none exist (S = 4^a (8b + 7))."""
    q = S
    while q and q % 4 == 0:
        q //= 4
    if q % 8 == 7:
        return None
    a = math.isqrt(S)
    while a >= 0:
        r = S - a * a
        b = math.isqrt(r)
        while 2 * b * b >= r:
            c = math.isqrt(r - b * b)
            if c * c == r - b * b:
                return a, b, c
            b -= 1
        a -= 1
    raise AssertionError(S)


def four_squares(S):
    a = math.isqrt(S)
    while three_squares(S - a * a) is None:
        a -= 1
    return (a,) + three_squares(S - a * a)


def squares(S):
    """Six integers whose squares sum to S: three for one mover and three for a second, the second's all zero where three squares
    exist, else a single small one."""
    three = three_squares(S)
    if three is not None:
        return three + (0, 0, 0)
    d = 1
    while three_squares(S - d * d) is None:
        d += 1
    return three_squares(S - d * d) + (d, 0, 0)


def split(S):
    """(a, 0, 0) for one mover and (x, y, z) != 0 for a second: a^2 + x^2 + y^2 + z^2 == S, a as large as that allows."""
    a = math.isqrt(S - 1)
    while three_squares(S - a * a) is None:
        a -= 1
    return (a, 0, 0), three_squares(S - a * a)


# ---- synthetic complexes ------------------------------------------------------------------------------------------------------

# rec_movers / lig_movers: backbone indices of the side, at most two
Spec = collections.namedtuple("Spec", "n_rec_bb n_lig_bb rec_movers lig_movers")
PITCH = 3.75


def bb_xyz(i):
    return PITCH * (i % 8), PITCH * ((i // 8) % 8), PITCH * (i // 64)


def side_atoms(n_bb, ligand):
    """(name, resname, element, residue number, x, y, z) in file order; the backbone atom of residue i is atom 3 i + 1."""
    if n_bb == 0:
        return [("N", "ALA", "N", 1, -0.5, 0.125, 0.0)]
    atoms = []
    for i in range(n_bb):
        x, y, z = bb_xyz(i)
        name, res, el = ("P", "DA", "P") if ligand and i % 3 == 2 else ("CA", "ALA", "C")
        atoms += [("N", res, "N", i + 1, x - 0.5, y + 0.125, z), (name, res, el, i + 1, x, y, z),
                  ("C", res, "C", i + 1, x + 0.5, y + 0.25, z + 0.125)]
    return atoms


def pdb_line(serial, name, resname, chain, seq, x, y, z, element):
    return "ATOM  %5d  %-3s %3s %1s%4d    %8.3f%8.3f%8.3f  1.00  0.00          %2s\n" % (serial, name, resname, chain, seq, x, y, z, element)


def side_modes(n_bb, movers):
    """(3 x movers, atoms, 3): mode 3 k + axis moves the backbone atom movers[k] by 1.0 along the axis; None without movers."""
    if not movers:
        return None
    modes = np.zeros((3 * len(movers), max(1, 3 * n_bb), 3))
    for k, p in enumerate(movers):
        assert 0 <= p < n_bb
        for axis in range(3):
            modes[3 * k + axis, 3 * p + 1, axis] = 1.0
    return modes


def write_complex(spec, directory):
    """The two PDB files in `directory` and the two mode arrays: (rec_pdb, lig_pdb, rec_modes, lig_modes)."""
    paths = []
    for side, (n_bb, chain) in enumerate(((spec.n_rec_bb, "A"), (spec.n_lig_bb, "B"))):
        path = os.path.join(directory, "%s_%d_%d.pdb" % ("lr"[side == 0], spec.n_rec_bb, spec.n_lig_bb))
        with open(path, "w") as f:
            for serial, (name, res, el, seq, x, y, z) in enumerate(side_atoms(n_bb, side == 1)):
                f.write(pdb_line(serial + 1, name, res, chain, seq, x, y, z, el))
        paths.append(path)
    return paths[0], paths[1], side_modes(spec.n_rec_bb, spec.rec_movers), side_modes(spec.n_lig_bb, spec.lig_movers)


def make_complex(pkg, spec, directory):
    rec, lig, rm, lm = write_complex(spec, directory)
    return pkg.Complex(rec, lig, rm, 0 if rm is None else len(rm), lm, 0 if lm is None else len(lm))


def pose_len(spec):
    return 7 + 3 * len(spec.rec_movers) + 3 * len(spec.lig_movers)


def movers_of(spec, measure):
    """The movers a measure sees, the ligand's first: (side, k), side 0 the receptor."""
    lig = [(1, k) for k in range(len(spec.lig_movers))]
    return lig + ([(0, k) for k in range(len(spec.rec_movers))] if measure == "complex" else [])


def pose_row(spec, moves=(), t=(0.0, 0.0, 0.0)):
    """The identity rotation, translation t (A), and the movers ((side, k), (dx, dy, dz)) displaced by integer thousandths."""
    row = np.zeros(pose_len(spec))
    row[:3] = t
    row[3] = 1.0
    for (side, k), d in moves:
        at = 7 + 3 * k + (3 * len(spec.rec_movers) if side == 1 else 0)
        row[at:at + 3] += np.array(d, dtype=np.float64) / 1000.0
    return row


def n_measured(spec, measure):
    return spec.n_lig_bb + (spec.n_rec_bb if measure == "complex" else 0)


def posed(spec, poses):
    """(poses, receptor then ligand backbone atoms, 3) f64 under the identity rotation: the device's operations on a mover, term
    by term (a mode that does not move an atom adds +-0.0 to it)."""
    poses = np.asarray(poses, dtype=np.float64)
    assert np.all(poses[:, 3] == 1.0) and not poses[:, 4:7].any()
    rec = np.broadcast_to(np.array([bb_xyz(i) for i in range(spec.n_rec_bb)]).reshape(-1, 3), (len(poses), spec.n_rec_bb, 3)).copy()
    lig = np.broadcast_to(np.array([bb_xyz(i) for i in range(spec.n_lig_bb)]).reshape(-1, 3), (len(poses), spec.n_lig_bb, 3)).copy()
    for k, p in enumerate(spec.rec_movers):
        for axis in range(3):
            rec[:, p, axis] = rec[:, p, axis] + 1.0 * poses[:, 7 + 3 * k + axis]
    base = 7 + 3 * len(spec.rec_movers)
    for k, p in enumerate(spec.lig_movers):
        for axis in range(3):
            lig[:, p, axis] = lig[:, p, axis] + 1.0 * poses[:, base + 3 * k + axis]
    lig = lig + poses[:, None, :3]
    return np.concatenate([rec, lig], axis=1)


def table(spec, poses, measure):
    """(poses, 3 x measured atoms) int64: the printed thousandths the measure compares."""
    X = posed(spec, poses)
    if measure == "ligand":
        X = X[:, spec.n_rec_bb:]
    return thousandths_of(X).reshape(len(poses), -1)


def expect(spec, poses, scoring, cutoff, measure):
    return bsas(table(spec, poses, measure), n_measured(spec, measure), scoring, cutoff)


# A case: `expected` maps each measure the case is built for to the oracle's (cluster_of, representatives, ties) of the whole list;
# `swarms` (swarms, glowworms) pose indices: the same poses as many small swarms of one ld_complex_cluster call (None: not asked);
# `intended` [(i, j, S)]: what the builder meant the integer S of poses i and j to be, under the first measure.
Case = collections.namedtuple("Case", "name spec poses scoring cutoff expected swarms intended")


def make_case(name, spec, rows, cutoff, measures, swarms=None, intended=(), scoring=None):
    poses = np.array(rows)
    scoring = 100.0 - np.arange(len(poses), dtype=np.float64) if scoring is None else np.asarray(scoring, dtype=np.float64)
    expected = {m: expect(spec, poses, scoring, cutoff, m) for m in measures}
    return Case(name, spec, poses, scoring, cutoff, expected, None if swarms is None else np.asarray(swarms), list(intended))


def swarm_expected(case, measure="complex"):
    """The oracle on every swarm of case.swarms: [(cluster_of, representatives, ties)]."""
    T = table(case.spec, case.poses, measure)
    n = n_measured(case.spec, measure)
    return [bsas(T[idx], n, case.scoring[idx], case.cutoff) for idx in case.swarms]


def place(spec, measure, six):
    """Six integers onto the first two movers of the measure (one mover takes three; None if the rest is not zero)."""
    movers = movers_of(spec, measure)
    moves = [(movers[0], six[:3])]
    if any(six[3:]):
        if len(movers) < 2:
            return None
        moves.append((movers[1], six[3:]))
    return moves


def filler(f):
    """Far-away pose f < 343: the first ligand mover on a 50 A lattice from (100, 100, 100) A, beyond every cutoff used with it."""
    assert f < 343
    return [((1, 0), (100000 + 50000 * (f % 7), 100000 + 50000 * ((f // 7) % 7), 100000 + 50000 * (f // 49)))]


# ---- a. threshold pairs -------------------------------------------------------------------------------------------------------

THRESHOLD_N = (1, 2, 31, 32, 33, 64, 65, 97)
CUTOFFS = (-1.0, 0.0, 0.0001, 0.5, 4.0, 30.0, INF)


def threshold_spec(n, measure):
    """n measured atoms: over the complex, half on either side with a mover each (two on the ligand where the receptor has none);
    over the ligand, a rigid receptor of three."""
    if measure == "ligand":
        return Spec(3, n, (), (0, n - 1) if n > 1 else (0,))
    n_rec = n // 2
    n_lig = n - n_rec
    if n_rec:
        return Spec(n_rec, n_lig, (n_rec - 1,), (0,))
    return Spec(0, n_lig, (), (0, n_lig - 1) if n_lig > 1 else (0,))


def probe_sums(n, cutoff):
    K = threshold_K(cutoff)
    if K is None:
        return [0, 1, 2, 3]
    if K == INF:
        return [0, 1, 10 ** 10, 4 * 10 ** 10]
    f = s_floor(n, cutoff)
    return [S for S in (f - 1, f, f + 1, f + 2) if S >= 0]


@functools.lru_cache(maxsize=None)
def threshold_cases(n, measure):
    """A case a cutoff: the representative at rest and a probe at each of probe_sums from it (one mover cannot realise a sum that
    is no sum of three squares: such a probe is left out, and never the one at floor(s*) or the one above)."""
    spec = threshold_spec(n, measure)
    cases = []
    for cutoff in CUTOFFS:
        rows, intended = [pose_row(spec)], []
        for S in probe_sums(n, cutoff):
            moves = place(spec, measure, squares(S))
            if moves is not None:
                intended.append((len(rows), 0, S))
                rows.append(pose_row(spec, moves))
        swarms = [[0, j] for j in range(1, len(rows))]
        cases.append(make_case("a-%s-n%d-c%r" % (measure, n, cutoff), spec, rows, cutoff, (measure,), swarms, intended))
    return cases


# ---- b. where the deciding term sits ------------------------------------------------------------------------------------------

# name -> Spec.  Index in complex_bsas's order (receptor first) | in the ranked walk (ligand first, receptor if it has modes):
LAYOUTS = {
    "one-granule":   Spec(12, 20, (0, 11), (0, 19)),     # 0, 11, 12, 31 | 20, 31, 0, 19: walk 32
    "last-single":   Spec(13, 20, (0, 12), (0, 19)),     # 0, 12, 13, 32 | 20, 32, 0, 19: walk 33, its last granule one atom
    "n65":           Spec(32, 33, (0, 31), (31, 32)),    # 0, 31, 63, 64 | 33, 64, 31, 32
    "n97-rec64":     Spec(64, 33, (32, 63), (0, 32)),    # 32, 63, 64, 96 | 65, 96, 0, 32
    "n97-lig64":     Spec(33, 64, (0, 32), (63, 31)),    # 0, 32, 96, 64 | 64, 96, 63, 31
    "rigid-rec-33":  Spec(13, 20, (), (0, 19)),          # 13, 32 | 0, 19: the receptor counts in n and is not walked
    "rigid-rec-97":  Spec(64, 33, (), (0, 32)),          # 64, 96 | 0, 32
}
WHERE_CUTOFF = 4.0
WHERE_FILLERS = (0, 63)


@functools.lru_cache(maxsize=None)
def where_case(layout, measure, fillers):
    """The representative, `fillers` far-away poses (63: the probes stand behind the first 64 candidates and ranked_sweep decides
    them), then for S = floor(s*) and floor(s*) + 1: the whole of S in each mover (a fourth square, where three do not exist, in
    the next mover), and S split over every ordered pair of movers, a single square in the first and three in the second."""
    spec = LAYOUTS[layout]
    f = s_floor(n_measured(spec, measure), WHERE_CUTOFF)
    movers = movers_of(spec, measure)
    rows = [pose_row(spec)] + [pose_row(spec, filler(i)) for i in range(fillers)]
    intended = []

    def add(moves, S):
        intended.append((len(rows), 0, S))
        rows.append(pose_row(spec, moves))

    for i, m in enumerate(movers):
        other = movers[(i + 1) % len(movers)]
        for S in (f, f + 1):
            six = squares(S)
            add([(m, six[:3]), (other, six[3:])], S)
    for m1 in movers:
        for m2 in movers:
            if m1 != m2:
                for S in (f, f + 1):
                    one, three = split(S)
                    add([(m1, one), (m2, three)], S)
    swarms = [[0, j] for j in range(1 + fillers, len(rows))] if fillers == 0 else None
    return make_case("b-%s-%s-f%d" % (layout, measure, fillers), spec, rows, WHERE_CUTOFF, (measure,), swarms, intended)


# ---- c. ranked-list positions -------------------------------------------------------------------------------------------------

POSITION_SPEC = LAYOUTS["last-single"]
POSITIONS = (64, 255, 256, 300)
POSITION_CUTOFF = 4.0


def shuffled(name, spec, rows, cutoff, measures, intended, seed):
    """The list handed over in another order than its scores': (case, position of every input index in the ranked order)."""
    n = len(rows)
    perm = np.random.default_rng(seed).permutation(n)          # input index i holds sorted position perm[i]
    inverse = np.argsort(perm)
    case = make_case(name, spec, [rows[p] for p in perm], cutoff, measures, None,
                     [(int(inverse[i]), int(inverse[j]), S) for i, j, S in intended], scoring=100.0 - perm)
    return case


@functools.lru_cache(maxsize=None)
def position_case(measure, pos):
    """The leader first, far-away fillers up to `pos`, then two probes at sorted positions pos and pos + 1: at floor(s*) and at
    floor(s*) + 1 from the leader, the one within first but at 255 and 300."""
    spec = POSITION_SPEC
    f = s_floor(n_measured(spec, measure), POSITION_CUTOFF)
    rows = [pose_row(spec)] + [pose_row(spec, filler(i)) for i in range(pos - 1)]
    intended = []
    for S in ((f + 1, f) if pos in (255, 300) else (f, f + 1)):
        intended.append((len(rows), 0, S))
        rows.append(pose_row(spec, place(spec, measure, squares(S))))
    return shuffled("c-%s-pos%d" % (measure, pos), spec, rows, POSITION_CUTOFF, (measure,), intended, pos)


@functools.lru_cache(maxsize=None)
def two_leader_case(measure, joins, fillers):
    """Leaders L1 at rest and L2 = the second ligand mover at (w, joins == 2, 0), w even and w^2 > s*, so that L2 is out of L1;
    the probe has that mover at (w / 2, joins == 2, b) and the first at p, b^2 + |p|^2 = floor(s*) - w^2 / 4: it is at floor(s*)
    from L2 and at floor(s*) + 1 (joins == 2: it joins the second) or floor(s*) (joins == 1: the first) from L1."""
    spec = POSITION_SPEC
    f = s_floor(n_measured(spec, measure), POSITION_CUTOFF)
    w = 2 * (math.isqrt(f) // 2 + 2)
    y = int(joins == 2)
    b, p1, p2, p3 = four_squares(f - w * w // 4)
    rows = [pose_row(spec), pose_row(spec, [((1, 1), (w, y, 0))])] + [pose_row(spec, filler(i)) for i in range(fillers)]
    probe = len(rows)
    rows.append(pose_row(spec, [((1, 1), (w // 2, y, b)), ((1, 0), (p1, p2, p3))]))
    intended = [(1, 0, w * w + y), (probe, 0, f + y), (probe, 1, f)]
    return shuffled("c-%s-joins%d-f%d" % (measure, joins, fillers), spec, rows, POSITION_CUTOFF, (measure,), intended, 7 + fillers)


# ---- d. half-thousandths ------------------------------------------------------------------------------------------------------

HALF_SPECS = {"ligand-atom": Spec(0, 1, (), ()), "receptor-mover": Spec(1, 0, (0,), ())}
HALF_K = (list(range(-150, 150)) + [s * (100000 + j) for s in (1, -1) for j in range(50)]
          + [s * (100000000 + j) for s in (1, -1) for j in range(50)])


def half_values():
    """[(k, t, lo, hi)]: t the double nearest (k + 0.5) / 1000, lo = k / 1000, hi = (k + 1) / 1000."""
    return [(k, (k + 0.5) / 1000.0, k / 1000.0, (k + 1) / 1000.0) for k in HALF_K]


@functools.lru_cache(maxsize=None)
def half_case(which):
    """One measured atom at the origin and cutoff 0.0: two poses share a cluster iff their printed thousandths are equal.  A swarm
    a k: the pose at t, then lo and hi; t prints as one of the two.  The axis turns with the k."""
    spec = HALF_SPECS[which]
    rows = []
    for i, (k, t, lo, hi) in enumerate(half_values()):
        for v in (t, lo, hi):
            row = pose_row(spec)
            row[(0 if which == "ligand-atom" else 7) + i % 3] = v
            rows.append(row)
    swarms = np.arange(len(rows)).reshape(-1, 3)
    measures = MEASURES if which == "ligand-atom" else ("complex",)
    return make_case("d-" + which, spec, rows, 0.0, measures, swarms)


# ---- e. range -----------------------------------------------------------------------------------------------------------------

LARGEST = 2147483.647      # prints as 2 147 483 647 thousandths, the largest accepted
REFUSED = 2147483.648


@functools.lru_cache(maxsize=None)
def range_cases(which):
    """Two poses at +-2.1e6 A on one axis, 4.2e9 thousandths apart (2^32 = 4.29e9): out at 4.0, in at 1e9; and a thousandth at
    exactly +-2 147 483 647 next to its neighbour."""
    spec = HALF_SPECS[which]
    at = 0 if which == "ligand-atom" else 7
    measures = MEASURES if which == "ligand-atom" else ("complex",)

    def rows(values):
        out = []
        for axis, v in values:
            row = pose_row(spec)
            row[at + axis] = v
            out.append(row)
        return out

    far = rows([(1, 2.1e6), (1, -2.1e6)])
    edge = rows([(2, LARGEST), (2, 2147483.646), (2, -LARGEST)])
    return [make_case("e-%s-far-4" % which, spec, far, 4.0, measures, [[0, 1]], [(1, 0, 4200000000 ** 2)]),
            make_case("e-%s-far-1e9" % which, spec, far, 1e9, measures, [[0, 1]], [(1, 0, 4200000000 ** 2)]),
            make_case("e-%s-largest" % which, spec, edge, 4.0, measures, [[0, 1, 2]], [(1, 0, 1), (2, 0, 4294967294 ** 2)])]


def refused_row(which):
    spec = HALF_SPECS[which]
    row = pose_row(spec)
    row[(0 if which == "ligand-atom" else 7) + 2] = REFUSED
    return row


# ---- every case ---------------------------------------------------------------------------------------------------------------

THRESHOLD_GROUPS = [(n, m) for n in THRESHOLD_N for m in MEASURES]
WHERE_GROUPS = [(layout, m) for layout in LAYOUTS for m in MEASURES]


def exact_cases():
    """The cases of a, b, c and e: every posed coordinate is an integer count of thousandths by construction."""
    for n, m in THRESHOLD_GROUPS:
        yield from threshold_cases(n, m)
    for layout, m in WHERE_GROUPS:
        for fillers in WHERE_FILLERS:
            yield where_case(layout, m, fillers)
    for m in MEASURES:
        for pos in POSITIONS:
            yield position_case(m, pos)
        for joins in (1, 2):
            for fillers in (0, 70):
                yield two_leader_case(m, joins, fillers)
    for which in HALF_SPECS:
        yield from range_cases(which)


def all_cases():
    yield from exact_cases()
    for which in HALF_SPECS:
        yield half_case(which)


# ---- ties: no oracle, the two calls against each other ------------------------------------------------------------------------

# (n, K): 400 S == n (2K + 1)^2 at S = (n / 16) ((2K + 1) / 5)^2, a perfect square, and the f64 expression of within_cutoff holds
# at S and fails at the next double above it (tests/test_bsas_edges_cpu.py): ranked_begin's bisection then ends ON the integer S.
# Off a tie s_max is never an integer -- s* is at least 1/400 from one and s_max within a few ulps of s* -- so only here does
# `S <= s_max` differ from `S < s_max` for an integer S.
TIES = ((16, 5002), (16, 100002), (64, 5002))


def float_path(S, n, cutoff):
    """within_cutoff of kernels/complex_pose.hpp, operation by operation in IEEE f64."""
    return bool(np.rint(np.sqrt(np.float64(S) * 1e-6 / np.float64(n)) * 1e4) / 1e4 <= cutoff)


def tie_cases():
    """[(spec, poses, scoring, cutoff, S)]: the representative and one pose at the tie from it, on the ligand's mover and on the
    receptor's.  No expectation: the float path decides a tie."""
    out = []
    for n, K in TIES:
        spec = Spec(n // 2, n // 2, (n // 2 - 1,), (0,))
        S = n * (2 * K + 1) ** 2 // 400
        d = math.isqrt(S)
        assert d * d == S
        for mover in movers_of(spec, "complex"):
            poses = np.array([pose_row(spec), pose_row(spec, [(mover, (0, d, 0))])])
            out.append((spec, poses, np.array([1.0, 0.0]), K / 1e4, S))
    return out
