"""Swarms that sit ON the knife edges of the GSO movement kernels' decisions (gso_step.hip: `gso_movement_phase`,
`gso_movement_phased`, `gso_move`, `qslerp`, `anm_step`): `l_i < l_j` at a tie, `d < vr` at d == vr and an ulp either side, the
vision range's clamps at 0 and 5 and the kFarD2 short cut, a glowworm that lands exactly on its target and then divides by a
zero norm, the roulette's order across the 64-bit words of the kept verdicts, the 4- and 8-wide tails of the scans, the slerp's
branches at dot == 0.9995, +-1 and +-0, and ANM steps whose squared norm is 0 or inf.  Shared by tests/test_gso_edges_cpu.py
(the oracle alone: every motif is ON its edge, and a restatement in plain Python floats gives the oracle's decisions bit for
bit) and tests/test_gpu_gso_edges.py (the kernels against the oracle, bit for bit).  No test functions here.

The complex "P": one receptor atom at the origin, one ligand atom at the origin of the ligand's frame -- a rotation cannot
change the energy -- scored by DFIRE with a STAIRCASE table: the one (receptor type, ligand type) row holds +-2^-k, k distinct
per bin, everything else 0.  A pose's energy is then the step function 4.7 - 0.0157 * v[bin(|t|)] of its translation: glowworms
in one bin tie exactly, glowworms in different bins differ, beyond 15 A everything scores 4.7.  (Powers of two: v * 0.0157 is
exact, so the tail of src/dfire.rs:347 gives the same bits whether or not a compiler fuses the multiply into the subtraction.)
The staircase is V-shaped, dimmest in bin 9 (6 <= |t| < 6.5): a glowworm there can have brighter neighbours on every side.
"P-anm" adds a receptor mode that moves the receptor atom along x by 2^-20 A per unit of extent (far below every margin here),
further receptor modes and all ligand modes with zero vectors: the extents evolve and move nothing.

A swarm is assembled from MOTIFS, groups of 2 to 10 glowworms more than 6 A from every other motif, padded with fillers beyond
40 A (they all score 4.7, tie, and are nobody's neighbour; half of them coincide) to chosen glowworm indices.  A motif is built
in a canonical frame -- the members of a pair differ in ONE coordinate and one of them has 0 there, so the difference the kernel
forms is the typed-in offset exactly -- at a radius found by a scan, so that its members fall into the bins it needs, at least MARGIN from
every bin edge; a signed permutation of the axes (|t| does not change) then puts it where there is room.

The launch arithmetic is restated by gso_shapes.launch(); every row of CASES spells out what it expects of it.
"""
import math
import os

import numpy as np

from gso_shapes import K2_ALL, launch  # noqa: F401  (launch: re-exported for the tests)
from setup_reference import chacha_block
from test_gpu_dfire_tables import ROW, TABLE_LEN, _DIST_TO_BINS, dyadic_ints
from test_gpu_parity import _write_pdb

NAN, INF = float("nan"), float("inf")
LINEAR_THRESHOLD = 0.9995        # src/constants.rs:11
FAR_D2 = 25.5                    # kFarD2 of gso_step.hip
KEPT_UP_TO = 256
STEPS = 20
MARGIN = 4e-4                    # angstrom between a motif's member and the nearest bin edge, at the start
SEPARATION = 6.0                 # angstrom between members of different motifs, at the start
DIMMEST_BIN = 9
MODE_X = 2.0 ** -20              # P-anm: the receptor atom's shift along x per unit of the first receptor extent


def below(x):
    return math.nextafter(x, -INF)


def above(x):
    return math.nextafter(x, INF)


# ---- the staircase -------------------------------------------------------------------------------------------------------

def rank_of_bin(b):
    """Brightness order of the bins: 0 dimmest (bin 9), growing to both sides, all distinct."""
    return 2 * abs(b - DIMMEST_BIN) + (1 if b > DIMMEST_BIN else 0)


def value_of_rank(r):
    """+2^-r for the 20 dimmest ranks, then -2^-(39 - r): strictly decreasing in r, so the energy 4.7 - 0.0157 v grows with r."""
    return 2.0 ** -r if r < 20 else -(2.0 ** -(39 - r))


def staircase(rec_type, lig_type):
    table = np.zeros(TABLE_LEN)
    for b in range(20):
        table[rec_type * ROW + lig_type * 20 + b] = value_of_rank(rank_of_bin(b))
    assert len(set(table[rec_type * ROW + lig_type * 20:][:20])) == 20
    dyadic_ints(table, 19)      # asserts: every value is a multiple of 2^-19
    return table


def bin_of(t):
    """(bin, angstrom to the nearest place where the index of src/dfire.rs:338 changes) of a translation, in f64 as the oracle."""
    x, y, z = t
    d2 = (0.0 - x) * (0.0 - x) + (0.0 - y) * (0.0 - y) + (0.0 - z) * (0.0 - z)
    if not d2 <= 225.0:
        return None, math.sqrt(d2) - 15.0
    d = math.sqrt(d2) * 2.0 - 1.0
    idx = int(max(d, 0.0))
    edge = min(d - idx, idx + 1 - d) / 2.0 if d > 0.0 else (0.0 - d) / 2.0
    return int(_DIST_TO_BINS[idx]) - 1, min(edge, (15.0 - math.sqrt(d2)))


def energy_of_bin(b):
    """src/dfire.rs:347 for the one pair (the restraint and membrane terms are 0, exactly)."""
    return 4.7 if b is None else (value_of_rank(rank_of_bin(b)) * 0.0157 - 4.7) * -1.0


# ---- plain-float restatement of the movement phase (src/glowworm.rs, src/swarm.rs, src/qt.rs) -------------------------------------

def fdiv(a, b):
    """IEEE a / b (Python raises on a zero divisor)."""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)


def fmin(a, b):
    return b if a != a else a if b != b else min(a, b)


def fmax(a, b):
    return b if a != a else a if b != b else max(a, b)


def fsqrt(x):
    return NAN if x != x or x < 0.0 else math.sqrt(x)


def fsin(x):
    return NAN if x != x or abs(x) == INF else math.sin(x)


def facos(x):
    return NAN if x != x or abs(x) > 1.0 else math.acos(x)


def q_normalize(q):                                              # src/qt.rs:40-46
    n = fsqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return [fdiv(c, n) for c in q]


def q_dot(a, b):
    """The dot of src/qt.rs:72 after its two normalisations."""
    q1, q2 = q_normalize(a), q_normalize(b)
    return q1[0] * q2[0] + q1[1] * q2[1] + q1[2] * q2[2] + q1[3] * q2[3]


def q_slerp(a, b, t, mutate=()):
    """src/qt.rs:67-91 -> (rotation, dot before the flip, flipped, branch "linear" | "slerp")."""
    q1, q2 = q_normalize(a), q_normalize(b)
    dot = q1[0] * q2[0] + q1[1] * q2[1] + q1[2] * q2[2] + q1[3] * q2[3]
    raw, flip = dot, dot < 0.0
    if flip:
        q1 = [-c for c in q1]
        dot *= -1.0
    if (dot >= LINEAR_THRESHOLD) if "dot>=" in mutate else (dot > LINEAR_THRESHOLD):
        return q_normalize([q1[k] + t * (q2[k] - q1[k]) for k in range(4)]), raw, flip, "linear"
    dot = fmax(fmin(dot, 1.0), -1.0)
    omega = facos(dot)
    so = fsin(omega)
    s1, s2 = fdiv(fsin((1.0 - t) * omega), so), fdiv(fsin(t * omega), so)
    return [s1 * q1[k] + s2 * q2[k] for k in range(4)], raw, flip, "slerp"


def anm_step(mine, other):
    """src/glowworm.rs:159-188 -> (extents, cum)."""
    cum, delta = 0.0, []
    for k in range(len(mine)):
        diff = other[k] - mine[k]
        delta.append(diff)
        cum += diff * diff
    coef = fdiv(0.5, fsqrt(cum))
    return [mine[k] + delta[k] * coef for k in range(len(mine))], cum


class Panic(Exception):
    """Where the reference indexes out of bounds (src/glowworm.rs:121-125)."""


class Draws:
    """Draw number step * N + i of the swarm's StdRng stream (src/swarm.rs:118): words 2 (k % 8), +1 of ChaCha block k / 8."""

    def __init__(self, key):
        self.key, self.blocks = [int(k) for k in key], {}

    def rnd(self, k):
        if k >> 3 not in self.blocks:
            self.blocks[k >> 3] = chacha_block(self.key, k >> 3)
        w = self.blocks[k >> 3]
        bits = (w[2 * (k & 7) + 1] << 32) | w[2 * (k & 7)]
        return float(bits >> 11) * (1.0 / 9007199254740992.0)


def restate_step(poses, vision, luciferin, draws, done, k_rec, k_lig, mutate=()):
    """One movement phase (src/swarm.rs:72-126) in Python floats: `poses`, `vision` before it, `luciferin` after the step's update,
    `done` steps before it.  -> (poses, vision, n_neighbors, target, moved, events); events[i] holds what the tests ask about.
    `mutate`: one of the kernel mutations of the issue, applied to the restatement."""
    n = len(poses)
    far = 24.9 if "far" in mutate else FAR_D2
    out_poses, out_vision, counts, targets, moved, events = [], [], [], [], [], {}
    for i in range(n):
        x1, y1, z1 = poses[i][:3]
        li, vr = luciferin[i], vision[i]
        nb, dist = [], {}
        for j in range(n):                                        # src/swarm.rs:87-100
            if j == i:
                continue
            lj = luciferin[j]
            if not ((li <= lj) if "li<=lj" in mutate else (li < lj)):
                continue
            x2, y2, z2 = poses[j][:3]
            d2 = (x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2) + (z1 - z2) * (z1 - z2)
            if d2 > far:
                continue
            d = fsqrt(d2)
            dist[j] = d
            if (d <= vr) if "d<=vr" in mutate else (d < vr):
                nb.append(j)
        cnt = len(nb)
        total, diffs = 0.0, []
        for j in nb:                                              # src/glowworm.rs:98-112
            diffs.append(luciferin[j] - li)
            total += diffs[-1]
        walk = nb
        if "&31" in mutate and n <= KEPT_UP_TO:                   # the kept verdicts, a bit a candidate, folded at 32
            walk = sorted({(j // 64) * 64 + ((j % 64) & 31) for j in nb})
        rnd = draws.rnd(done * n + i)                             # one draw per glowworm, src/swarm.rs:118
        chosen, ev = i, dict(cnt=cnt, rnd=rnd, neighbors=nb, nearest=dist)
        if cnt > 0:                                               # src/glowworm.rs:114-126
            s, k, before = 0.0, 0, 0.0
            while s < rnd:
                if k >= len(walk):
                    raise Panic("glowworm %d: the probabilities sum to %r < %r" % (i, s, rnd))
                before = s
                s += fdiv(luciferin[walk[k]] - li, total)
                k += 1
            if k == 0:
                raise Panic("glowworm %d: rnd == 0" % i)
            chosen = walk[k - 1]
            ev.update(place=k - 1, margin=min(s - rnd, rnd - before), luciferins=[luciferin[j] for j in nb])
        row = list(poses[i])
        if chosen != i:                                           # src/glowworm.rs:128-190
            other = poses[chosen]
            dx, dy, dz = other[0] - row[0], other[1] - row[1], other[2] - row[2]
            norm = fsqrt(dx * dx + dy * dy + dz * dz)
            coef = fdiv(0.5, norm)
            row[0], row[1], row[2] = row[0] + dx * coef, row[1] + dy * coef, row[2] + dz * coef
            row[3:7], dot, flip, branch = q_slerp(poses[i][3:7], other[3:7], 0.5, mutate)
            ev.update(norm=norm, coef=coef, dot=dot, flip=flip, branch=branch)
            if k_rec:
                row[7:7 + k_rec], ev["cum_rec"] = anm_step(poses[i][7:7 + k_rec], other[7:7 + k_rec])
            if k_lig:
                row[7 + k_rec:], ev["cum_lig"] = anm_step(poses[i][7 + k_rec:], other[7 + k_rec:])
        v = vr + 0.08 * float(5 - cnt)                            # src/glowworm.rs:91-96
        out_vision.append(fmin(5.0, v if "nofmax" in mutate else fmax(0.0, v)))
        out_poses.append(row)
        counts.append(cnt)
        targets.append(chosen)
        moved.append(1 if chosen != i else 0)
        events[i] = ev
    return out_poses, out_vision, counts, targets, moved, events


def same_bits(a, b):
    """Equal bit for bit, NaNs of any payload equal in place, +0 and -0 NOT equal."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)))


# ---- the values on the edges, computed and not typed in -------------------------------------------------------------------------

def quiet_vision(k):
    """The vision range after k movement phases without a neighbour: v0 = 0.2, v(k+1) = min(5, max(0, vk + 0.08 * 5))."""
    v = 0.2
    for _ in range(k):
        v = min(5.0, max(0.0, v + 0.08 * float(5 - 0)))
    return v


def first_quiet_phase_at_5():
    k = 0
    while quiet_vision(k) != 5.0:
        k += 1
    return k


def around_far_d2():
    """Offsets D with D * D just below, at (if a double's square rounds there) and just above kFarD2."""
    d = math.sqrt(FAR_D2)
    while d * d >= FAR_D2:
        d = below(d)
    out = {"farlo": d}
    d = above(d)
    if d * d == FAR_D2:
        out["farat"] = d
        while d * d == FAR_D2:
            d = above(d)
    out["farhi"] = d
    assert out["farlo"] * out["farlo"] < FAR_D2 < out["farhi"] * out["farhi"]
    return out


def _search_dot(want):
    """A unit-ish target (c, s, 0, 0) whose dot with the mover (1, 0, 0, 0), as qslerp computes it, is `want` exactly."""
    c = want
    for _ in range(4000):
        q = [c, math.sqrt(1.0 - c * c), 0.0, 0.0]
        got = q_dot([1.0, 0.0, 0.0, 0.0], q)
        if got == want:
            return q
        c = above(c) if got < want else below(c)
    raise AssertionError("no target quaternion gives dot %r" % want)


def rotations():
    """name -> (mover's rotation, target's rotation, dot, branch, flipped): the slerp's edges (E9)."""
    one = [1.0, 0.0, 0.0, 0.0]
    half = [0.5, 0.5, 0.5, 0.5]
    out = {
        "eq": (one, _search_dot(LINEAR_THRESHOLD), LINEAR_THRESHOLD, "slerp", False),
        "next": (one, _search_dot(above(LINEAR_THRESHOLD)), above(LINEAR_THRESHOLD), "linear", False),
        "one": (half, half, 1.0, "linear", False),
        "anti": (half, [-0.5, -0.5, -0.5, -0.5], -1.0, "linear", True),
        "zero": (one, [0.0, 1.0, 0.0, 0.0], 0.0, "slerp", False),
        "negzero": ([1.0, -0.0, -0.0, -0.0], [-0.0, 1.0, 0.0, 0.0], -0.0, "slerp", False),
        "neg": (one, [-0.6, 0.8, 0.0, 0.0], None, "slerp", True),
        "norm2": (one, [1.2, 1.6, 0.0, 0.0], None, "slerp", False),
    }
    for name, (a, b, dot, branch, flip) in out.items():
        got = q_dot(a, b)
        if dot is not None:
            assert got == dot and math.copysign(1.0, got) == math.copysign(1.0, dot), (name, got)
        assert (got < 0.0) == flip and ((abs(got) > LINEAR_THRESHOLD) == (branch == "linear")), (name, got)
    return out


# E10: (mover's extents, target's) of a side of k modes, by kind
def extents(kind, k):
    rest = [0.25] * (k - 1)
    first = {"unit": (0.0, 1.0), "unitneg": (0.25, -0.75), "same": (0.5, 0.5), "tiny": (0.0, 1e-170), "huge": (0.0, 1e200)}[kind]
    return [first[0]] + rest, [first[1]] + rest


# name -> (receptor side, ligand side, cum of the receptor side, cum of the ligand side)
ANM_SETTINGS = {
    "half": ("unit", "unitneg", 1.0, 1.0),          # one-mode rows: the steps are +0.5 and -0.5 exactly
    "recsame": ("same", "unit", 0.0, 1.0),          # cum = 0: 0.5 / 0 = inf, 0 * inf = NaN
    "ligsame": ("unit", "same", 1.0, 0.0),
    "tiny": ("unit", "tiny", 1.0, 0.0),             # 1e-170 squared underflows: cum = 0, the step is 1e-170 * inf = inf
    "huge": ("unit", "huge", 1.0, INF),             # 1e200 squared overflows: cum = inf, coef = 0, no step
}


# ---- motifs -------------------------------------------------------------------------------------------------------------------

def _landing(y_from, y_to):
    """Where a glowworm at y_from lands that moves towards y_to, in the kernel's operations."""
    dy = y_to - y_from
    return y_from + dy * (0.5 / math.sqrt(dy * dy))


CROWD_Y = ((0.6, 0.45), (0.3, 0.45))   # (seeker, crowd): moving inwards (|t| falls: for r < 6) and outwards (for r > 6.5)
FAN_A = 1.87                       # fan: the seeker's distance to each neighbour (first inside the vision range at phase 6: 2.2)
FAN_U = [c / math.sqrt(14.0) for c in (1.0, 2.0, 3.0)]
PHIS = (0.0, 0.9, 1.8, 2.7, 3.6, 4.5, 5.4)


def motif_offsets(kind, arg=None):
    """Variants of a motif: its members' offsets along the motif's axis (y in the canonical frame) from a base in the x-z plane."""
    if kind == "tie":                  # E1: one bin, 0.1 A apart
        return [[0.0, 0.1]]
    if kind == "pair":                 # E2-E4, E6: dy = -D exactly, d = sqrt(D * D)
        return [[0.0, arg]]
    if kind == "crowd":                # E5: a seeker and `arg` coincident brighter neighbours 0.15 A away; with 8 of them a
        out = []                       # brighter glowworm exactly where the seeker lands
        for seeker, crowd in CROWD_Y:
            out.append([seeker] + [crowd] * arg + ([_landing(seeker, crowd)] if arg == 8 else []))
        return out
    raise KeyError(kind)


def fan_members(r, vertices):
    s = [r * u for u in FAN_U]
    out = [tuple(s)]
    for v in vertices:
        p = list(s)
        p[v // 2] += FAN_A if v % 2 == 0 else -FAN_A
        out.append(tuple(p))
    return out


def _ranks(points):
    out = []
    for p in points:
        b, edge = bin_of(p)
        if b is None or edge < MARGIN:
            return None
        out.append(rank_of_bin(b))
    return out


def _want(kind, ranks):
    if kind == "tie":
        return ranks[0] == ranks[1]
    if kind == "pair":
        return ranks[0] != ranks[1]
    if kind == "crowd":
        return all(r > ranks[0] for r in ranks[1:])
    if kind == "fan":
        return all(r > ranks[0] for r in ranks[1:]) and len(set(ranks)) == len(ranks)
    raise KeyError(kind)


_CANON = {}


def canonical(kind, arg=None):
    """Candidate member lists of a motif in the canonical frame, on radii where its members fall into the bins it needs."""
    key = (kind, arg)
    if key not in _CANON:
        found = []
        if kind == "fan":
            for r in np.arange(5.0, 8.0, 1.0 / 256):
                m = fan_members(float(r), arg)
                ranks = _ranks(m)
                if ranks and _want(kind, ranks):
                    found.append(m)
        else:
            grid = np.arange(2.0, 13.5, 1.0 / 2048)
            for ys in motif_offsets(kind, arg):
                # a first look in numpy: no member within 2 MARGIN of a half-integer of 2 |t| - 1; then every 0.3 A the real test
                ok = np.ones(len(grid), dtype=bool)
                for y in set(ys):
                    d = np.sqrt(grid * grid + y * y) * 2.0 - 1.0
                    ok &= np.abs(d - np.rint(d)) > 4.0 * MARGIN
                last = -1.0
                for r in grid[ok]:
                    if r - last < 0.3:
                        continue
                    ranks = _ranks([(float(r), y, 0.0) for y in ys])
                    if not ranks or not _want(kind, ranks):
                        continue
                    last = float(r)
                    for phi in PHIS:
                        m = [(last * math.cos(phi), y, last * math.sin(phi)) for y in ys]
                        if _ranks(m) == ranks:
                            found.append(m)
        assert found, key
        _CANON[key] = found
    return _CANON[key]


_ISOMETRIES = [(p, s) for p in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
               for s in ((1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1), (-1, 1, 1), (-1, 1, -1), (-1, -1, 1), (-1, -1, -1))]


def _apply(iso, p):
    perm, sign = iso
    return tuple(sign[k] * p[perm[k]] for k in range(3))


def place(placed, candidates, rng):
    """The first candidate (in a seeded order), under one of the 48 signed permutations of the axes, that keeps SEPARATION from
    everything placed so far.  -x is exact, so the differences of the members stay what they were."""
    have = np.array(placed).reshape(-1, 3)
    for c in rng.permutation(len(candidates) * 48)[:6000]:
        m = [_apply(_ISOMETRIES[c % 48], p) for p in candidates[c // 48]]
        if len(have) == 0 or np.min(np.linalg.norm(have[None, :, :] - np.array(m)[:, None, :], axis=2)) >= SEPARATION:
            return m
    raise AssertionError("no room for a motif")


# ---- cases ---------------------------------------------------------------------------------------------------------------------
# A motif: (name, kind, arg, glowworm indices of its members in member order, rotation setting or None, ANM setting or
# None).  Members: tie / pair: the one at 0, the one at the offset; crowd: seeker, neighbours, (landing); fan: seeker, neighbours.

def _pair(name, d, idx, rot=None, anm=None):
    return (name, "pair", d, idx, rot, anm)


def _e2(i, rot="eq"):       # three pairs straddling a bin step at D = 0.2 and an ulp either side; the one inside moves at phase 1
    return [_pair("E2at", 0.2, (i, i + 1)), _pair("E2in", below(0.2), (i + 2, i + 3), rot), _pair("E2out", above(0.2), (i + 4, i + 5))]


def _e3(i):                 # D = v2 and an ulp inside: neighbours first at phases 4 and 3
    return [_pair("E3at", quiet_vision(2), (i, i + 1), "next"), _pair("E3in", below(quiet_vision(2)), (i + 2, i + 3), "one")]


def _e4(i):
    far = around_far_d2()
    out = [_pair("E4at", 5.0, (i, i + 1)), _pair("E4in", below(5.0), (i + 2, i + 3), "anti"), _pair("E4far", 5.04, (i + 4, i + 5))]
    for k, name in enumerate(sorted(far)):
        out.append(_pair("E4" + name, far[name], (i + 6 + 2 * k, i + 7 + 2 * k)))
    return out


def _e5(i):                 # 5, 6, 7, 8 neighbours at phase 1: 31 glowworms
    out, rots = [], {5: "zero", 6: "negzero", 7: "neg", 8: "norm2"}
    for c in (5, 6, 7, 8):
        size = 1 + c + (1 if c == 8 else 0)
        out.append(("E5x%d" % c, "crowd", c, tuple(range(i, i + size)), rots[c], None))
        i += size
    return out


def _fan(name, seeker, neighbours):
    vertices = {2: (0, 5), 3: (0, 3, 5), 6: (0, 1, 2, 3, 4, 5)}[len(neighbours)]
    return (name, "fan", vertices, (seeker,) + tuple(neighbours), None, None)


def _movers(i, settings):   # P-anm: pairs that move at phase 1, one per ANM setting
    return [_pair("E10" + s, below(0.2), (i + 2 * k, i + 2 * k + 1), None, s) for k, s in enumerate(settings)]


CASES = {
    # the smallest swarm with a neighbour: the pair an ulp inside 0.2; its seeker is glowworm 1 = N - 1 (the CPU test asserts it)
    "N2": dict(S=1, N=2, modes=None, seed=2, motifs=[_pair("E2in", below(0.2), (0, 1), "eq")],
               expect={None: dict(kernel="phased", parts=1, share=2, threads=64, lds=96, words=1),
                       "single": dict(kernel="single", parts=1, share=2, threads=64, lds=64, words=1),
                       "phased": dict(kernel="phased", threads=64, lds=96)}),
    # one partly filled trip of 8 lanes a glowworm: 9 * 8 = 72 lanes -> 128 threads
    "N9": dict(S=1, N=9, modes=None, seed=9, motifs=[("E1", "tie", None, (0, 8), None, None)] + _e2(1),
               expect={None: dict(kernel="phased", parts=1, share=9, threads=128, lds=432, words=1),
                       "single": dict(kernel="single", threads=64, lds=288, words=1), "phased": dict(kernel="phased", threads=128)}),
    # N mod 4 = 1, N mod 8 = 1; parts = min(ceil(65/64) = 2, 512) = 2, share 33: 264 lanes -> 320 threads; two words of verdicts.
    # The fan's neighbours are N-3, N-2, N-1 = 62, 63, 64: across the word boundary, in both scans' tails
    "N65": dict(S=1, N=65, modes=None, seed=65,
                motifs=[_fan("E7x3", 5, (62, 63, 64))] + _e5(6) + _e3(40) + [_pair("E6", 0.5, (50, 51))],
                expect={None: dict(kernel="phased", parts=2, share=33, threads=320, lds=3120, words=2, trips=[[33], [32]]),
                        "single": dict(kernel="single", parts=2, share=33, threads=64, lds=2080, words=2),
                        "phased": dict(kernel="phased", threads=320)}),
    # N mod 4 = 2: neighbours 63, 64, 65
    "N66": dict(S=1, N=66, modes=None, seed=66,
                motifs=[_fan("E7x3", 7, (63, 64, 65)), ("E1", "tie", None, (0, 62), None, None)] + _e2(10, "neg") + _e4(20),
                expect={None: dict(kernel="phased", parts=2, share=33, threads=320, lds=3168, words=2),
                        "single": dict(kernel="single", threads=64, lds=2112, words=2), "phased": dict(kernel="phased")}),
    # N mod 4 = 3, N mod 8 = 3: neighbours 64, 65, 66 of seeker 63; a fan across the first word boundary (2 and 62 of seeker 1)
    "N67": dict(S=1, N=67, modes=None, seed=67,
                motifs=[_fan("E7x3", 63, (64, 65, 66)), _fan("E7x2", 1, (2, 62))] + _e5(10) + [_pair("E6", 0.5, (50, 51))] + _e3(52),
                expect={None: dict(kernel="phased", parts=2, share=34, threads=320, lds=3216, words=2, trips=[[34], [33]]),
                        "single": dict(kernel="single", parts=2, share=34, threads=64, lds=2144, words=2),
                        "phased": dict(kernel="phased")}),
    # the last size that keeps verdict bits: four full words.  parts = 4, share 64: 512 threads
    "N256": dict(S=1, N=256, modes=None, seed=256,
                 motifs=[_fan("E7x2", 10, (63, 64)), _fan("E7x3", 11, (127, 128, 130)), _fan("E7x6", 12, (189, 190, 191, 192, 254, 255)),
                         ("E1", "tie", None, (0, 1), None, None)] + _e2(20) + _e3(30) + _e4(40) + _e5(65)
                 + [_pair("E6", 0.5, (100, 101))],
                 expect={None: dict(kernel="phased", parts=4, share=64, threads=512, lds=12288, words=4, second_walk=False),
                         "single": dict(kernel="single", parts=4, share=64, threads=64, lds=8192, words=4),
                         "phased": dict(kernel="phased", threads=512)}),
    # the first size on the second walk: parts = 5, share = ceil(257/5) = 52: 416 lanes -> 448 threads; seeker 256 = N - 1,
    # its neighbours N - 2, N - 3; the phased kernel's last trip of 8 candidates is 256 alone
    "N257": dict(S=1, N=257, modes=None, seed=257,
                 motifs=[_fan("E7x2", 256, (254, 255)), _fan("E7x3", 63, (64, 128, 200)), ("E1", "tie", None, (0, 1), None, None)]
                 + _e2(20) + _e3(30) + [_pair("E6", 0.5, (100, 101))] + _e5(130),
                 expect={None: dict(kernel="phased", parts=5, share=52, threads=448, lds=12336, words=0, second_walk=True),
                         "single": dict(kernel="single", parts=5, share=52, threads=64, lds=8224, second_walk=True),
                         "phased": dict(kernel="phased", threads=448)}),
    # N mod 8 = 7: parts = 5, share 53
    "N263": dict(S=1, N=263, modes=None, seed=263,
                 motifs=[_fan("E7x3", 255, (260, 261, 262)), _fan("E7x6", 12, (63, 64, 127, 128, 192, 259))] + _e4(40) + _e2(20)
                 + [("E1", "tie", None, (0, 1), None, None)],
                 expect={None: dict(kernel="phased", parts=5, share=53, threads=448, lds=12624, second_walk=True),
                         "single": dict(kernel="single", threads=64, lds=8416, second_walk=True), "phased": dict(kernel="phased")}),
    # 600 copies of the N = 67 swarm with seeds of their own: parts = min(2, max(1, ceil(512/600) = 1)) = 1, a share of 67:
    # 536 lanes -> 576 threads; 40 200 glowworms: the phased kernel is the launch's own choice
    "M67": dict(S=600, N=67, modes=None, seed=600, like="N67",
                expect={None: dict(kernel="phased", parts=1, share=67, threads=576, lds=3216, words=2, trips=[[67]]),
                        "single": dict(kernel="single", parts=1, share=67, threads=128, lds=2144),
                        "phased": dict(kernel="phased", parts=1)}),
    # P-anm, 1 + 1 modes: the steps of a one-mode row; kept verdicts
    "A11": dict(S=1, N=12, modes=(1, 1), seed=11, motifs=_movers(0, ("half", "recsame", "ligsame", "tiny", "huge")),
                expect={None: dict(kernel="phased", parts=1, share=12, threads=128, lds=576, words=1),
                        "single": dict(kernel="single", threads=64, lds=384), "phased": dict(kernel="phased")}),
    # P-anm, 3 + 2 modes, on the second walk
    "A32": dict(S=1, N=261, modes=(3, 2), seed=32, motifs=_movers(250, ("half", "recsame", "ligsame", "tiny", "huge")),
                expect={None: dict(kernel="phased", parts=5, share=53, threads=448, lds=12528, second_walk=True),
                        "single": dict(kernel="single", lds=8352), "phased": dict(kernel="phased")}),
    # ... and in a swarm that keeps its verdicts
    "A32k": dict(S=1, N=12, modes=(3, 2), seed=33, motifs=_movers(1, ("half", "recsame", "ligsame", "tiny", "huge")),
                 expect={None: dict(kernel="phased", words=1), "single": dict(kernel="single"), "phased": dict(kernel="phased")}),
}
KEPT = [c for c in CASES if CASES[c]["N"] <= KEPT_UP_TO]
SECOND_WALK = [c for c in CASES if CASES[c]["N"] > KEPT_UP_TO]


def motifs_of(case):
    c = CASES[case]
    return CASES[c["like"]]["motifs"] if "like" in c else c["motifs"]


def sampled_swarms(case):
    s = CASES[case]["S"]
    return (0,) if s == 1 else (0, s // 2, s - 1)


def build_swarm(case):
    """(positions (N, pose_len), {motif name: glowworm indices}) of a case's swarm."""
    c = CASES[case]
    n = c["N"]
    k_rec, k_lig = c["modes"] or (0, 0)
    rows = np.zeros((n, 7 + k_rec + k_lig))
    rows[:, 3] = 1.0
    for i in range(n):                   # fillers: odd ones coincide, even ones 1 A apart along a line
        rows[i, :3] = (50.0, 0.0, 0.0) if i % 2 else (60.0 + i // 2, 0.0, 0.0)
    rng = np.random.default_rng(7 + (CASES[c["like"]]["seed"] if "like" in c else c["seed"]))
    placed, where, taken = [], {}, set()
    rot = rotations()
    for name, kind, arg, idx, rot_name, anm_name in motifs_of(case):
        members = place(placed, canonical(kind, arg), rng)
        assert len(members) == len(idx) and not taken & set(idx) and max(idx) < n, (case, name)
        taken |= set(idx)
        placed += members
        where[name] = tuple(idx)
        ranks = _ranks(members)
        for i, p in zip(idx, members):
            rows[i, :3] = p
        mover = idx[0] if kind in ("crowd", "fan") or ranks[0] < ranks[1] else idx[1]
        for i in idx:
            if rot_name:
                rows[i, 3:7] = rot[rot_name][0 if i == mover else 1]
            if anm_name:
                rec_kind, lig_kind = ANM_SETTINGS[anm_name][:2]
                rows[i, 7:7 + k_rec] = extents(rec_kind, k_rec)[0 if i == mover else 1]
                rows[i, 7 + k_rec:] = extents(lig_kind, k_lig)[0 if i == mover else 1]
        where[name + ":mover"] = mover
    return rows, where


class Edges:
    """The complexes P and P-anm, the cases' swarms, oracle scorers and replays, and the restatement's events; made once."""

    def __init__(self, pkg, orc, directory):
        self.pkg, self.orc = pkg, orc
        self.rec, self.lig = os.path.join(directory, "P_rec.pdb"), os.path.join(directory, "P_lig.pdb")
        _write_pdb(self.rec, [("N", "ALA", "A", 1, 0.0, 0.0, 0.0)])
        _write_pdb(self.lig, [("N", "GLY", "B", 1, 0.0, 0.0, 0.0)])
        probe = orc.Scorer("dfire", self.rec, self.lig, potential=np.zeros(TABLE_LEN))
        assert probe.num_atoms(0) == 1 and probe.num_atoms(1) == 1
        self.table = staircase(int(probe.model(0)["dfire_types"][0]), int(probe.model(1)["dfire_types"][0]))
        self._cpu, self._hip, self._swarms, self._replays, self._restated = {}, {}, {}, {}, {}

    def scorer_kwargs(self, modes):
        kw = dict(potential=self.table)
        if modes is not None:
            k_rec, k_lig = modes
            rec_modes = np.zeros((k_rec, 1, 3))
            rec_modes[0, 0, 0] = MODE_X
            kw.update(use_anm=True, rec_num_anm=k_rec, lig_num_anm=k_lig, rec_nmodes=rec_modes.ravel(),
                      lig_nmodes=np.zeros((k_lig, 1, 3)).ravel())
        return kw

    def cpu(self, modes):
        if modes not in self._cpu:
            self._cpu[modes] = self.orc.Scorer("dfire", self.rec, self.lig, **self.scorer_kwargs(modes))
        return self._cpu[modes]

    def hip(self, modes):
        if modes not in self._hip:
            self._hip[modes] = self.pkg.Scorer.from_pdb("dfire", self.rec, self.lig, **self.scorer_kwargs(modes))
        return self._hip[modes]

    def swarm(self, case):
        if case not in self._swarms:
            self._swarms[case] = build_swarm(case)
        return self._swarms[case]

    def swarms(self, case):
        """(positions (S, N, pose_len), seeds (S,) uint64): S copies of the swarm, every one its own seed, the seed of swarm 1
        again at S - 1."""
        c = CASES[case]
        rows, _ = self.swarm(case)
        positions = np.ascontiguousarray(np.broadcast_to(rows, (c["S"],) + rows.shape))
        seeds = (np.arange(c["S"]) + 1000 * c["seed"] + 324324).astype(np.uint64)
        if c["S"] > 1:
            seeds[c["S"] - 1] = seeds[1]
        return positions, seeds

    def replay(self, case):
        """{swarm: [state before the first step, after step 1, ...]} of the oracle for the sampled swarms; the last state
        carries "num_evals"."""
        if case not in self._replays:
            c = CASES[case]
            positions, seeds = self.swarms(case)
            out = {}
            for s in sampled_swarms(case):
                ref = self.orc.GSO(self.cpu(c["modes"]), positions[s], seed=int(seeds[s]))
                states = [ref.state()]
                for _ in range(STEPS):
                    ref.step()
                    states.append(ref.state())
                states[-1]["num_evals"] = ref.num_evals
                out[s] = states
            self._replays[case] = out
        return self._replays[case]

    def restate(self, case, swarm=0, mutate=()):
        """[(poses, vision, n_neighbors, target, moved, events) per step] of the restatement, each step from the ORACLE's state
        before it (poses, vision range) and the oracle's luciferins after its update."""
        key = (case, swarm, tuple(mutate))
        if key not in self._restated:
            c = CASES[case]
            states = self.replay(case)[swarm]
            k_rec, k_lig = c["modes"] or (0, 0)
            draws = Draws(self.pkg.stdrng_key(int(self.swarms(case)[1][swarm])))
            out = []
            for step in range(1, STEPS + 1):
                before, after = states[step - 1], states[step]
                out.append(restate_step(before["poses"].tolist(), before["vision_range"].tolist(), after["luciferin"].tolist(),
                                        draws, step - 1, k_rec, k_lig, mutate))
            self._restated[key] = out
        return self._restated[key]

    def agrees(self, case, swarm, restated):
        """None if the restatement's decisions, vision ranges and poses are the oracle's bit for bit (NaNs in place; rotations
        of the slerp branch, which go through libm, to 1e-12), else what differs first."""
        states = self.replay(case)[swarm]
        for step, (poses, vision, counts, targets, moved, events) in enumerate(restated, 1):
            want = states[step]
            for name, got in (("n_neighbors", counts), ("target", targets), ("moved", moved)):
                if not np.array_equal(np.array(got), want[name]):
                    return "step %d: %s" % (step, name)
            if not same_bits(vision, want["vision_range"]):
                return "step %d: vision_range" % step
            got = np.array(poses)
            cols = np.r_[0:3, 7:got.shape[1]]
            if not same_bits(got[:, cols], want["poses"][:, cols]):
                return "step %d: translations or extents" % step
            for i, ev in events.items():
                if ev.get("branch") == "slerp":
                    if not np.array_equal(np.isnan(got[i, 3:7]), np.isnan(want["poses"][i, 3:7])) or \
                       not np.nanmax(np.abs(got[i, 3:7] - want["poses"][i, 3:7]), initial=0.0) < 1e-12:
                        return "step %d: rotation of %d (slerp)" % (step, i)
                elif not same_bits(got[i, 3:7], want["poses"][i, 3:7]):
                    return "step %d: rotation of %d" % (step, i)
        return None


_shared = None


def edges(pkg, orc, directory):
    """One Edges per test session: both test modules replay the oracle once."""
    global _shared
    if _shared is None:
        _shared = Edges(pkg, orc, directory)
    return _shared
