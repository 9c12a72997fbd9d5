"""The rule of include/lightdock_hip.h, "Preparing a run"  restated from the text in int64 numpy and plain
Python floats, with a ChaCha block of its own: the checker of tests/test_prepare_cpu.py and tests/test_gpu_prepare.py.
Rules 1-3 are exact integers (every term below 2^53, well inside int64); rule 5 is IEEE doubles, operation by operation
in the order the header states, so only libm's ln can differ from the library."""
import math

import numpy as np

from sasa_reference import radius, records  # noqa: F401

LIMIT = 2000000
BEAD_RADIUS = 2000
MASK = 0xffffffff


# --- rule 1 ------------------------------------------------------------------------------------------------------------

def diameter2(xyz):
    """max |x_i - x_j|^2 of (n, 3) integers."""
    xyz = np.asarray(xyz, dtype=np.int64).reshape(-1, 3)
    best = 0
    for lo in range(0, len(xyz), 512):
        d = xyz[lo:lo + 512, None, :] - xyz[None, :, :]
        best = max(best, int((d * d).sum(axis=2).max()))
    return best


def distance(d2):
    """D = isqrt(d2) / 4, floor both times."""
    return math.isqrt(int(d2)) // 4


# --- rule 2 ------------------------------------------------------------------------------------------------------------

def lattice(atoms, h):
    """Per axis (first index, count): floor((min c - E_max - h) / h) .. ceil((max c + E_max + h) / h)."""
    atoms = np.asarray(atoms, dtype=np.int64).reshape(-1, 4)
    e_max = int(atoms[:, 3].max())
    axes = []
    for c in range(3):
        first = (int(atoms[:, c].min()) - e_max - h) // h
        last = -((-(int(atoms[:, c].max()) + e_max + h)) // h)
        axes.append((first, last - first + 1))
    return axes


def shell(atoms, bead=None, h=2000):
    """(candidates (count, 3) int64 in lexicographic order, lattice nodes)."""
    atoms = np.asarray(atoms, dtype=np.int64).reshape(-1, 4)
    bead = np.zeros(len(atoms), dtype=bool) if bead is None else np.asarray(bead, dtype=bool)
    (x0, nx), (y0, ny), (z0, nz) = lattice(atoms, h)
    ys, zs = (y0 + np.arange(ny, dtype=np.int64)) * h, (z0 + np.arange(nz, dtype=np.int64)) * h
    e2, reach2 = atoms[:, 3] ** 2, (atoms[:, 3] + h) ** 2
    out = []
    for i in range(nx):          # a plane of nodes at a time: every node against every atom
        x = (x0 + i) * h
        outside = np.ones((ny, nz), dtype=bool)
        near = np.zeros((ny, nz), dtype=bool)
        for b in range(len(atoms)):
            d2 = (x - atoms[b, 0]) ** 2 + ((ys - atoms[b, 1]) ** 2)[:, None] + ((zs - atoms[b, 2]) ** 2)[None, :]
            outside &= d2 >= e2[b]
            if not bead[b]:
                near |= d2 < reach2[b]
        j, k = np.nonzero(outside & near)    # row-major: j, then k ascending
        out.append(np.stack([np.full(len(j), x, dtype=np.int64), ys[j], zs[k]], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 3), dtype=np.int64), nx * ny * nz


# --- rule 3 ------------------------------------------------------------------------------------------------------------

def centres(points, max_centres, cover=0):
    """(indices, gap2) of farthest-point sampling: np.argmax returns the lowest index of a maximum."""
    p = np.asarray(points, dtype=np.int64).reshape(-1, 3)
    index, gap2 = [], []
    if len(p) == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    value = (p * p).sum(axis=1)          # the first pick is by |p|^2
    gap = np.full(len(p), np.iinfo(np.int64).max, dtype=np.int64)
    while len(index) < min(max_centres, len(p)):
        i = int(np.argmax(value))
        if value[i] < 0:
            break
        if index and cover > 0 and value[i] <= cover * cover:
            break
        index.append(i)
        gap2.append(int(value[i]))
        d = p - p[i]
        gap = np.minimum(gap, (d * d).sum(axis=1))
        gap[index] = -1                  # chosen: out of the running
        value = gap
    return np.array(index, dtype=np.int64), np.array(gap2, dtype=np.int64)


# --- rule 4 ------------------------------------------------------------------------------------------------------------

def restraint_filter(centre_points, restraint_points, per_restraint):
    """Indices, ascending, of the centres among the per_restraint nearest to some restraint point (ties by index)."""
    c = np.asarray(centre_points, dtype=np.int64).reshape(-1, 3)
    keep = set()
    for r in np.asarray(restraint_points, dtype=np.int64).reshape(-1, 3):
        d2 = ((c - r) ** 2).sum(axis=1)
        keep.update(sorted(range(len(c)), key=lambda i: (int(d2[i]), i))[:per_restraint])
    return sorted(keep)


# --- rule 5 ------------------------------------------------------------------------------------------------------------

def pcg32_key(seed):
    """rand_core 0.5 SeedableRng::seed_from_u64: eight key words."""
    mul, inc, m64 = 6364136223846793005, 11634580027462260723, (1 << 64) - 1
    state, key = seed & m64, []
    for _ in range(8):
        state = (state * mul + inc) & m64
        x = (((state >> 18) ^ state) >> 27) & MASK
        rot = state >> 59
        key.append(((x >> rot) | (x << ((32 - rot) & 31))) & MASK if rot else x)
    return key


def chacha_block(key, counter):
    def rotl(v, n):
        return ((v << n) & MASK) | (v >> (32 - n))
    s = [0x61707865, 0x3320646e, 0x79622d32, 0x6b206574] + [int(k) for k in key] + [counter & MASK, (counter >> 32) & MASK, 0, 0]
    x = list(s)

    def qr(a, b, c, d):
        x[a] = (x[a] + x[b]) & MASK; x[d] = rotl(x[d] ^ x[a], 16)
        x[c] = (x[c] + x[d]) & MASK; x[b] = rotl(x[b] ^ x[c], 12)
        x[a] = (x[a] + x[b]) & MASK; x[d] = rotl(x[d] ^ x[a], 8)
        x[c] = (x[c] + x[d]) & MASK; x[b] = rotl(x[b] ^ x[c], 7)
    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    return [(a + b) & MASK for a, b in zip(x, s)]


class Draws:
    """The draws ((s G + g) << 16) + j of one row."""

    def __init__(self, key, s, g, glowworms):
        self.key, self.base, self.used, self.blocks = key, ((s * glowworms + g) << 16), 0, {}

    def v(self):
        return 2.0 * self.u() - 1.0

    def u(self):
        k = self.base + self.used
        self.used += 1
        if k // 8 not in self.blocks:
            self.blocks[k // 8] = chacha_block(self.key, k // 8)
        w = self.blocks[k // 8]
        bits = (w[2 * (k % 8) + 1] << 32) | w[2 * (k % 8)]
        return float(bits >> 11) * 2.0 ** -53


def norm3(v):
    return math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def arc_rotation(l, d):
    """(w, x, y, z) taking unit(l) to unit(d) by the shortest arc."""
    nl, nd = norm3(l), norm3(d)
    if not nl > 0.0 or not nd > 0.0:
        return [1.0, 0.0, 0.0, 0.0]
    a, b = [c / nl for c in l], [c / nd for c in d]
    w = 1.0 + ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2])
    if w < 1e-12:
        axis = min(range(3), key=lambda c: (abs(a[c]), c))
        c = cross(a, [1.0 if k == axis else 0.0 for k in range(3)])
        nc = norm3(c)
        return [0.0] + [v / nc for v in c]
    c = cross(a, b)
    nq = math.sqrt(((w * w + c[0] * c[0]) + c[1] * c[1]) + c[2] * c[2])
    return [w / nq] + [v / nq for v in c]


def pose_row(seed, glowworms, s, g, centre, radius=10.0, rec_points=(), lig_points=(), anm_rec=0, anm_lig=0, key=None):
    """(row, draws consumed)."""
    d = Draws(pcg32_key(seed) if key is None else key, s, g, glowworms)
    while True:
        v = [d.v(), d.v(), d.v()]
        if (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2] <= 1.0:
            break
    t = [centre[c] + radius * v[c] for c in range(3)]
    if len(rec_points) and len(lig_points):
        ir = min(int(math.floor(d.u() * len(rec_points))), len(rec_points) - 1)
        il = min(int(math.floor(d.u() * len(lig_points))), len(lig_points) - 1)
        q = arc_rotation([float(c) for c in lig_points[il]], [float(rec_points[ir][c]) - t[c] for c in range(3)])
    else:
        while True:
            x1, y1 = d.v(), d.v()
            r1 = x1 * x1 + y1 * y1
            if r1 < 1.0:
                break
        while True:
            x2, y2 = d.v(), d.v()
            r2 = x2 * x2 + y2 * y2
            if 0.0 < r2 < 1.0:
                break
        scale = math.sqrt((1.0 - r1) / r2)
        q = [x1, y1, x2 * scale, y2 * scale]
    extents = []
    while len(extents) < anm_rec + anm_lig:
        while True:
            v1, v2 = d.v(), d.v()
            sq = v1 * v1 + v2 * v2
            if 0.0 < sq < 1.0:
                break
        f = math.sqrt((-2.0 * math.log(sq)) / sq)
        extents += [v1 * f, v2 * f]
    return t + q + extents[:anm_rec + anm_lig], d.used


def rotate(q, v):
    """The vector v turned by the unit quaternion q = (w, x, y, z)."""
    w, u = q[0], q[1:]
    c1 = cross(u, v)
    c1 = [c1[k] + w * v[k] for k in range(3)]
    c2 = cross(u, c1)
    return [v[k] + 2.0 * c2[k] for k in range(3)]


# --- the cleaned files ---------------------------------------------------------------------------------------------------

def clean_records(path, keep_h=False, keep_oxt=False, keep_waters=False):
    """The records the cleaner keeps."""
    out = []
    for r in records(path):
        res, name = r[17:20].strip(), r[12:16].strip()
        if res != "MMB" and radius(r) == 0 and not keep_h:
            continue
        if name == "OXT" and not keep_oxt:
            continue
        if res in ("HOH", "WAT") and not keep_waters:
            continue
        out.append(r)
    return out


def thousandths_of(recs):
    return np.array([[int(round(float(r[30 + 8 * c:38 + 8 * c]) * 1000.0)) for c in range(3)] for r in recs], dtype=np.int64).reshape(-1, 3)


def centred(t):
    """floor((2 (t n - S) + n) / (2 n)) per axis."""
    t = np.asarray(t, dtype=np.int64)
    n = len(t)
    return (2 * (t * n - t.sum(axis=0)) + n) // (2 * n)


def shell_atoms(recs, D):
    """(atoms (m, 4) x y z E, bead flags) of a cleaned file's records: atoms with a radius and MMB beads."""
    t = thousandths_of(recs)
    atoms, bead = [], []
    for r, c in zip(recs, t):
        is_bead = r[17:20].strip() == "MMB"
        R = BEAD_RADIUS if is_bead else radius(r)
        if R > 0:
            atoms.append([int(c[0]), int(c[1]), int(c[2]), R + D])
            bead.append(is_bead)
    return np.array(atoms, dtype=np.int64).reshape(-1, 4), np.array(bead, dtype=bool)
