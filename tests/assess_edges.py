"""Model quality (ld_complex_assess, kernels/assess.hip and assess.hpp; lightdock_hip.h, "Model quality") at its edges: the
constructions and the high-precision reference of tests/test_assess_edges_cpu.py and tests/test_gpu_assess_edges.py.  No test
functions here.

Every case is a complex small enough to hold by hand, written from integer thousandths so that every number prints exactly:
a receptor file, a ligand file, and the two files of a reference whose records are matched by key and may sit in any frame.
A model is the receptor file as written plus the ligand under the identity quaternion and a translation that is a multiple of
0.001 A, so the posed thousandths are integers by construction (model_thousandths), whatever the f64 posing does.

The reference measure (reference_measures) works in mpmath at 60 digits on the exact integer sums: Horn's 4 x 4, mpmath.eigsy,
i-RMSD^2 from the largest eigenvalue (test_assess_cpu.exact_fit stays the authority for it), L-RMSD^2 from the top
eigenvector's rotation, and kappa = max |lambda_k| / (lambda_1 - lambda_2) of the RECEPTOR's superposition, inf at equality.

Bounds (bounds).  i-RMSD^2: the project's 64 eps (G_a + G_b) / n, unscaled at every gap -- the result is a Rayleigh quotient,
second order in the eigenvector's error.  L-RMSD^2: 128 eps (G_l,a + G_l,b) / n_l (1 + kappa): the error of the rotation found
is at most c eps max|lambda| / (lambda_1 - lambda_2), and it moves tr(R C) by at most |dR| sqrt(G_l,a G_l,b) <=
|dR| (G_l,a + G_l,b) / 2; 64 and 128 are the constants of tests/test_assess_cpu.py, the factor is derived here and is within
2 of the existing bound at kappa = 1.  kappa = inf: L-RMSD is unspecified; it must be finite, non-negative and at most
(sqrt(G_l,a / n_l) + sqrt(G_l,b / n_l))^2 (lrmsd_cap).

A coordinate field holds 8 columns: "%8.3f" prints down to -999.999 only.  Below that the field is written with two decimals
and the thousandths are a multiple of 10 (field); the parser and the restatement read the columns' number either way.
For the same reason of range the aliasing distances stop at 3 998 000, so that the other atom of the ligand's residue stays
within 2000 A, and the receptor turned by 1e-6 rad is spread over 1700 A: nearer the axis no thousandth would move."""
import functools
import os

import mpmath
import numpy as np

from test_assess_cpu import EPS, FRAME_Q, AssessRestated, exact_sums, moved, pdb_line, quaternion_matrix
from test_contacts_cpu import atom_contacts

DIGITS = 60
DEGENERATE = mpmath.mpf(10) ** -45        # a relative gap below this is equality: an integer matrix has no such gap by accident
FIT_CYCLE = ("N", "CA", "C", "O", "P")


# ---- files from integer thousandths -----------------------------------------------------------------------------

def field(t):
    t = int(t)
    s = "%8.3f" % (t / 1000.0)
    if len(s) > 8:
        assert t % 10 == 0, t
        s = "%8.2f" % (t / 1000.0)
    assert len(s) == 8 and int(round(float(s) * 1000.0)) == t, (t, s)
    return s


def atom(name, resname, chain, seq, xyz):
    return (name, resname, chain, int(seq), tuple(int(v) for v in xyz))


def atom_line(serial, a):
    name, resname, chain, seq, xyz = a
    line = pdb_line(serial, name if len(name) == 4 or name[0].isdigit() else " " + name, resname, chain, seq, (0.0, 0.0, 0.0))
    return line[:30] + "".join(field(v) for v in xyz) + line[54:]


def singles(points, chain, resname="ALA"):
    """Every point a residue of its own holding one fit atom, the names in turn."""
    return [atom(FIT_CYCLE[i % 5], resname, chain, i + 1, p) for i, p in enumerate(points)]


def with_xyz(atoms, points):
    return [atom(a[0], a[1], a[2], a[3], p) for a, p in zip(atoms, points)]


def xyz_of(atoms):
    return np.array([a[4] for a in atoms], dtype=np.int64).reshape(-1, 3)


class Case:
    """rec, lig: the model's files; ref_rec, ref_lig: the reference's (lists of atom()); poses: ligand translations in integer
    thousandths; C, I: contact and interface cutoff in thousandths; expect: what the CPU test confirms of the case."""

    def __init__(self, name, rec, lig, ref_rec, ref_lig, poses=((0, 0, 0),), C=5000, I=10000, **expect):
        self.name, self.rec, self.lig, self.ref_rec, self.ref_lig = name, list(rec), list(lig), list(ref_rec), list(ref_lig)
        self.poses, self.C, self.I, self.expect = [tuple(int(v) for v in p) for p in poses], C, I, expect

    @property
    def rows(self):
        return np.array([[p[0] / 1000.0, p[1] / 1000.0, p[2] / 1000.0, 1.0, 0.0, 0.0, 0.0] for p in self.poses])

    def model_thousandths(self, k):
        return np.concatenate([xyz_of(self.rec), xyz_of(self.lig) + np.array(self.poses[k], dtype=np.int64)])


class Built:
    """A case written to `directory` and restated."""

    def __init__(self, case, directory):
        self.case = case
        self.paths = []
        for side, atoms in (("rec", case.rec), ("lig", case.lig), ("ref_rec", case.ref_rec), ("ref_lig", case.ref_lig)):
            self.paths.append(os.path.join(directory, "%s_%s.pdb" % (case.name, side)))
            with open(self.paths[-1], "w") as f:
                f.write("".join(atom_line(i + 1, a) for i, a in enumerate(atoms)))
        self.rs = AssessRestated(self.paths[0], self.paths[1], None, None, self.paths[2], self.paths[3], case.C / 1000.0, case.I / 1000.0)
        self._measures = {}

    def measures(self, k):
        """The reference's measures of pose k: reference_measures' dict and kept, computed once a translation."""
        key = self.case.poses[k]
        if key not in self._measures:
            rs, t = self.rs, self.case.model_thousandths(k)
            m = reference_measures(t[rs.rec_fit], rs.ref_t[rs.rec_fit], t[rs.lig_fit], rs.ref_t[rs.lig_fit],
                                   t[rs.interface_fit], rs.ref_t[rs.interface_fit])
            m["kept"] = sum(bool(atom_contacts(t[a], t[b], rs.cutoff).any()) for a, b in rs.pair_atoms)
            self._measures[key] = m
        return self._measures[key]


@functools.lru_cache(maxsize=None)
def _built(case, directory):
    return Built(case, directory)


def built(case, directory):
    return _built(case, str(directory))


# ---- the reference measure --------------------------------------------------------------------------------------

def horn(S):
    (xx, xy, xz), (yx, yy, yz), (zx, zy, zz) = S
    return [[xx + yy + zz, yz - zy, zx - xz, xy - yx], [yz - zy, xx - yy - zz, xy + yx, zx + xz],
            [zx - xz, xy + yx, -xx + yy - zz, yz + zy], [xy - yx, zx + xz, yz + zy, -xx - yy + zz]]


def rotation(q):
    """The matrix R of the unit quaternion q = (w, x, y, z): R m ~ r for the top eigenvector of Horn's matrix of sum m r^T."""
    w, x, y, z = q
    return [[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]]


def spectrum(m, r):
    """int64 thousandths -> (n, G_m, G_r, eigenvalues of Horn's matrix in descending order, the top eigenvector, kappa), in
    thousandths^2, mpmath numbers at the precision in force."""
    n, A, B, K = exact_sums(m, r)
    S = [[mpmath.mpf(K[a][b]) / n for b in range(3)] for a in range(3)]
    E, Q = mpmath.eigsy(mpmath.matrix(horn(S)))
    order = sorted(range(4), key=lambda k: E[k], reverse=True)
    lam = [E[k] for k in order]
    q = [Q[i, order[0]] for i in range(4)]
    norm = mpmath.sqrt(sum(v * v for v in q))
    top = max(abs(v) for v in lam)
    gap = lam[0] - lam[1]
    kappa = mpmath.inf if top == 0 or gap <= top * DEGENERATE else top / gap
    return n, mpmath.mpf(A) / n, mpmath.mpf(B) / n, lam, [v / norm for v in q], kappa


def reference_measures(m_rec, r_rec, m_lig, r_lig, m_int, r_int):
    """int64 (n, 3) thousandths of the model's and the reference's receptor fit atoms, ligand fit atoms and interface fit atoms
    -> dict: irmsd2, ga, gb, lrmsd2, gla, glb (A^2, the G's as AssessRestated.bounds takes them), n_int, n_lig, kappa (float, inf
    at equality), lambdas (the receptor's four eigenvalues over the largest magnitude, floats), q (its top eigenvector) and
    lambda_int (n times the interface's largest eigenvalue, 55 digits as text: a root of test_assess_cpu.exact_fit's quartic)."""
    with mpmath.workdps(DIGITS):
        e6 = mpmath.mpf(10) ** 6
        n_int, ga, gb, lam, _, _ = spectrum(m_int, r_int)
        lam_int = lam[0]
        irmsd2 = max(mpmath.mpf(0), (ga + gb - 2 * lam_int) / n_int)
        n_rec, _, _, lam, q, kappa = spectrum(m_rec, r_rec)
        R = rotation(q)
        cm = [mpmath.mpf(int(m_rec[:, a].sum())) / n_rec for a in range(3)]
        cr = [mpmath.mpf(int(r_rec[:, a].sum())) / n_rec for a in range(3)]
        total = gla = glb = mpmath.mpf(0)
        for p, t in zip(m_lig.tolist(), r_lig.tolist()):
            x = [p[a] - cm[a] for a in range(3)]
            y = [t[a] - cr[a] for a in range(3)]
            d = [R[b][0] * x[0] + R[b][1] * x[1] + R[b][2] * x[2] - y[b] for b in range(3)]
            total += d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
            gla += x[0] * x[0] + x[1] * x[1] + x[2] * x[2]
            glb += y[0] * y[0] + y[1] * y[1] + y[2] * y[2]
        top = max(abs(v) for v in lam)
        return {"irmsd2": float(irmsd2 / e6), "ga": float(ga / e6), "gb": float(gb / e6), "n_int": n_int,
                "lrmsd2": float(total / len(m_lig) / e6), "gla": float(gla / e6), "glb": float(glb / e6), "n_lig": len(m_lig),
                "kappa": float(kappa), "lambdas": [float(v / top) if top != 0 else 0.0 for v in lam],
                "q": [float(v) for v in q], "lambda_int": mpmath.nstr(lam_int * n_int, 55)}


def bounds(m):
    """(bound on i-RMSD^2, bound on L-RMSD^2 or None where it is unspecified) in A^2 for a reference_measures dict."""
    bi = 64 * EPS * (m["ga"] + m["gb"]) / m["n_int"]
    bl = None if np.isinf(m["kappa"]) else 128 * EPS * (m["gla"] + m["glb"]) / m["n_lig"] * (1.0 + m["kappa"])
    return bi, bl


def lrmsd_cap(m):
    return (np.sqrt(m["gla"] / m["n_lig"]) + np.sqrt(m["glb"] / m["n_lig"])) ** 2


# ---- solver cases -----------------------------------------------------------------------------------------------

def cycled(p):
    """(x, y, z) -> (y, z, x): a proper rotation that keeps integers."""
    p = np.asarray(p, dtype=np.int64)
    return np.stack([p[..., 1], p[..., 2], p[..., 0]], axis=-1)


def solver_case(name, rec_m, lig_m, rec_r, lig_r, **kw):
    rec, lig = singles(rec_m, "A"), singles(lig_m, "B", "SER")
    return Case(name, rec, lig, with_xyz(rec, rec_r), with_xyz(lig, lig_r), **kw)


LINE = np.array([1, 2, 2], dtype=np.int64)                  # length 3
ACROSS = np.array([0, 1, -1], dtype=np.int64)               # perpendicular to it
LADDER_WIDTHS = (1000, 100, 10, 1)
LIGAND4 = np.array([[0, 3000, -3000], [1500, 4200, -2500], [300, 5600, -3300], [-900, 4300, -4800]], dtype=np.int64)   # chiral
LIGAND_NOISE = np.array([[120, -80, 40], [-60, 150, 90], [200, 10, -130], [-110, -70, 60]], dtype=np.int64)
ALONG_NOISE = np.array([30, -70, 110, -20, 50, -90, 40, -50, 80, -10, 60, -100, 20, -30, 90, -60], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def ladder_case(width):
    """16 receptor fit atoms 3.9 A apart on a line along (1, 2, 2), each `width` thousandths to one side of it or the other in y
    and z; the reference in a frame turned by (x, y, z) -> (y, z, x), shifted, its atoms moved ALONG the line by up to 0.3 A, so
    that its width is the model's.  sigma_1 = 340 * 3900^2, sigma_2 = 32 width^2, sigma_3 = 0: kappa ~ 8.1e7 / width^2."""
    base = np.array([10000, 20000, 30000], dtype=np.int64)
    sign = np.array([1, -1, -1, 1] * 4, dtype=np.int64)        # sum s_i = sum i s_i = 0: no cross term in S
    rec_m = base + np.arange(16)[:, None] * 1300 * LINE + sign[:, None] * width * ACROSS
    lig_m = rec_m[0] - sign[0] * width * ACROSS + LIGAND4
    shift = np.array([55000, -7000, 21000], dtype=np.int64)
    rec_r = cycled(rec_m + ALONG_NOISE[:, None] * LINE) + shift
    lig_r = cycled(lig_m + LIGAND_NOISE) + shift
    expect = {"kappa": None if width == 0 else 340 * 3900.0 ** 2 / (64.0 * width * width) + 0.5, "rank_one": "rec" if width == 0 else None}
    return solver_case("ladder_%d" % width, rec_m, lig_m, rec_r, lig_r, **expect)


@functools.lru_cache(maxsize=None)
def collinear_interface_case():
    """The six interface fit atoms (three a side) on a line in the model, a chiral arrangement in the reference: S of the
    interface has rank 1 and its top eigenvalue is double.  Three more receptor fit atoms, beyond the interface cutoff of the
    ligand, keep the receptor's own fit unique."""
    far = np.array([[30000, 0, 0], [30000, 4000, 1000], [33000, 1000, 5000]], dtype=np.int64)
    rec_r = np.concatenate([[[0, 0, 0], [3000, 1000, 0], [1000, 3500, 1200]], far]) + 50000
    lig_r = np.array([[0, 3000, -3000], [-2500, 2000, -1500], [-1000, -2000, -3500]], dtype=np.int64) + 50000
    rec_m = np.concatenate([[[0, 0, 0], [1000, 2000, 2000], [2500, 5000, 5000]], far + [[300, 100, -200], [-100, 100, 100], [100, -100, -200]]]) + 20000
    lig_m = np.array([[-1000, -2000, -2000], [-2200, -4400, -4400], [-3100, -6200, -6200]], dtype=np.int64) + 20000
    return solver_case("collinear_interface", rec_m, lig_m, rec_r, lig_r, rank_one="int")


@functools.lru_cache(maxsize=None)
def zero_s_case():
    """The interface's S is 0 exactly: the reference has r1, r2 on the receptor and -r1, -r2 on the ligand about a centre, and
    in the model each such pair coincides.  All four eigenvalues are 0 and i-RMSD^2 = (G_a + G_b) / n."""
    c = np.array([40000, 40000, 40000], dtype=np.int64)
    r1, r2 = np.array([2000, 1000, 0], dtype=np.int64), np.array([-1000, 1500, 1500], dtype=np.int64)
    far = np.array([[30000, 0, 0], [30000, 4000, 1000], [33000, 1000, 5000]], dtype=np.int64)
    rec_r, lig_r = np.concatenate([[c + r1, c + r2], c + far]), np.array([c - r1, c - r2])
    m1, m2 = np.array([7000, 1000, 3000], dtype=np.int64), np.array([9000, 4500, 2000], dtype=np.int64)
    rec_m = np.concatenate([[m1, m2], far + np.array([[200, -100, 50], [-150, 80, 120], [60, 90, -210]]) + 8000])
    lig_m = np.array([m1, m2])
    return solver_case("zero_s", rec_m, lig_m, rec_r, lig_r, zero_s=True)


CHIRAL6 = np.array([[0, 0, 0], [1458, 0, 0], [2009, 1420, 0], [1600, 2100, 950], [4100, -1300, 2200], [-2100, 3300, 4400]], dtype=np.int64)


def axis_turn(axis, angle):
    """Rodrigues' matrix, in longdouble rounded to f64: the reference is whatever `moved` prints of it."""
    n = np.asarray(axis, dtype=np.longdouble)
    n = n / np.sqrt((n * n).sum())
    Kx = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]], dtype=np.longdouble)
    a = np.longdouble(angle)
    return np.asarray(np.eye(3, dtype=np.longdouble) + np.sin(a) * Kx + (1 - np.cos(a)) * (Kx @ Kx), dtype=np.float64)


TURNS = {"half_110": ((1, 1, 0), np.pi), "half_122": ((1, 2, 2), np.pi), "half_236": ((2, -3, 6), np.pi),
         "half_plus": ((1, 2, 2), np.pi + np.pi / 180e3), "half_minus": ((1, 2, 2), np.pi - np.pi / 180e3),
         "micro": ((2, -3, 6), 1e-6)}


@functools.lru_cache(maxsize=None)
def turned_case(which):
    """A chiral complex against itself in a frame turned by a proper rotation: by 180 degrees about a direction that is no axis
    (q_0 = 0, the other components mixed), by 180 +- 0.001 degrees, by 1e-6 rad (the receptor spread over 1700 A there).  The reference is test_assess_cpu.moved's
    reprint of the model's records."""
    axis, angle = TURNS[which]
    spread = 400 if which == "micro" else 1            # 1e-6 rad moves an atom by a thousandth only 1000 A from the axis
    rec_m, lig_m = CHIRAL6 * spread + 30000, CHIRAL6[0] + 30000 + LIGAND4
    rec, lig = singles(rec_m, "A"), singles(lig_m, "B", "SER")
    R, t = axis_turn(axis, angle), np.array([150.0, 160.0, 170.0])

    def reprinted(atoms):
        lines = moved([atom_line(i + 1, a).rstrip("\n") for i, a in enumerate(atoms)], R, t)
        return with_xyz(atoms, [[int(round(float(l[30 + 8 * k:38 + 8 * k]) * 1000.0)) for k in range(3)] for l in lines])

    return Case("turned_" + which, rec, lig, reprinted(rec), reprinted(lig), turned=True)


@functools.lru_cache(maxsize=None)
def mirror_case():
    """The mirror image (z -> -z) of a chiral complex: not a fit."""
    rec_m, lig_m = CHIRAL6 + 30000, CHIRAL6[0] + 30000 + LIGAND4
    flip = np.array([1, 1, -1], dtype=np.int64)
    return solver_case("mirror", rec_m, lig_m, rec_m * flip + 90000, lig_m * flip + 90000, mirror=True)


MIRROR_D = (1000, 30, 1)


@functools.lru_cache(maxsize=None)
def mirror_family_case(d):
    """Six receptor fit atoms at (+-3000, 0, 0), (0, +-2000, 0), (0, 0, +-2000) against their mirror image: S = diag(s1, s2, -s2),
    the best proper rotation is not unique.  The atom on +z moved out by d thousandths (in the model and, mirrored, in the
    reference) opens the gap: the second and third singular values differ by about 5/3 * 2000 d.  The reference's frame is
    turned by (x, y, z) -> (y, z, x) besides, so that Horn's matrix is not diagonal."""
    pts = np.array([[3000, 0, 0], [-3000, 0, 0], [0, 2000, 0], [0, -2000, 0], [0, 0, 2000 + d], [0, 0, -2000]], dtype=np.int64)
    lig = pts[0] + LIGAND4
    flip = np.array([1, 1, -1], dtype=np.int64)
    return solver_case("mirror_family_%d" % d, pts + 30000, lig + 30000, cycled(pts * flip) + 90000, cycled(lig * flip) + 90000, mirror=True)


@functools.lru_cache(maxsize=None)
def perfect_far_case():
    """Twelve receptor fit atoms spread over +-1900 A (mean 0 exactly), a ligand fit atom 3 A from each, the reference equal to the
    model: every pair native, every atom in the interface, the true RMSD^2 of both measures 0, G ~ 1e8 A^2."""
    half = np.array([[1900000, -1234560, 777770], [-1500000, 1900000, -312340], [654320, 1111110, -1900000],
                     [1899990, 1899990, 1899990], [-1900000, 1900000, 123450], [10, -20, 1899000]], dtype=np.int64)
    rec = np.concatenate([half, -half])
    lig = rec + np.array([3000, 0, 0], dtype=np.int64) * np.where(rec[:, :1] > 0, -1, 1)
    return solver_case("perfect_far", rec, lig, rec, lig, perfect=True)


@functools.lru_cache(maxsize=None)
def corner_case():
    """The receptor file within 5 A of (+1990, -1990, +1990) A, the ligand posed next to it from near the origin; the reference
    in another frame near (-1500, +1500, -1500) A with about 1 A of noise.  G about the centroids stays near 1e2 A^2 while
    every raw sum is near its largest: the n sum|m|^2 - |sum m|^2 cancellation and assess_to_double where they matter."""
    rng = np.random.default_rng(20)
    corner = np.array([1990000, -1990000, 1990000], dtype=np.int64)
    rec_off = np.concatenate([[[0, 0, 0]], rng.integers(-280, 281, size=(9, 3)) * 10])
    lig_off = np.concatenate([[[2000, 1000, -1000]], rng.integers(-280, 281, size=(5, 3)) * 10 + np.array([3000, 2000, -2000])])
    home = np.array([5000, 5000, 5000], dtype=np.int64)
    pose = corner - home
    R = quaternion_matrix(FRAME_Q)

    def framed(off):
        noise = rng.integers(-100, 101, size=off.shape) * 10
        noise[0] = 0                                          # the native pair stays one
        return np.rint((off @ R.T) / 10.0).astype(np.int64) * 10 + noise + np.array([-1500000, 1500000, -1500000])

    rec_r, lig_r = framed(rec_off), framed(lig_off)
    return solver_case("corner", corner + rec_off, home + lig_off, rec_r, lig_r, poses=[tuple(pose)], corner=True)


@functools.lru_cache(maxsize=None)
def spread_case():
    """4096 fit atoms a side (1024 residues of N, CA, C, O each, a residue's atoms anywhere), uniform over +-1990 A in multiples of
    0.01 A, the reference the model with up to 2 A of noise a coordinate: sums near 2^55, n * sum near 2^67.  One pose."""
    rng = np.random.default_rng(4096)

    def cloud():
        p = rng.integers(-199000, 199001, size=(4096, 3)) * 10
        return np.clip(p - np.rint(p.mean(axis=0) / 10.0).astype(np.int64) * 10, -1990000, 1990000)

    rec_m, lig_m = cloud(), cloud()
    rec_m[0] = (100000, 200000, 300000)
    lig_m[0] = rec_m[0] + (3000, 0, 0)
    rec_r, lig_r = (p + rng.integers(-200, 201, size=p.shape) * 10 for p in (rec_m, lig_m))
    rec_r[0], lig_r[0] = rec_m[0], lig_m[0]
    rec = [atom(FIT_CYCLE[i % 4], "ALA", "A", i // 4 + 1, p) for i, p in enumerate(rec_m)]
    lig = [atom(FIT_CYCLE[i % 4], "SER", "B", i // 4 + 1, p) for i, p in enumerate(lig_m)]
    return Case("spread_4096", rec, lig, with_xyz(rec, rec_r), with_xyz(lig, lig_r), spread=True)


def solver_cases():
    cases = [ladder_case(w) for w in LADDER_WIDTHS + (0,)] + [collinear_interface_case(), zero_s_case()]
    cases += [turned_case(k) for k in sorted(TURNS)] + [mirror_case()] + [mirror_family_case(d) for d in MIRROR_D]
    return cases + [perfect_far_case(), corner_case()]


# ---- sums-kernel cases ------------------------------------------------------------------------------------------

FILL_NAMES = ("N", "CA", "C", "O", "CB", "HA", "CG", "1HB", "CD", "2HB", "OG", "HG", "CE", "1HD", "NZ", "2HD", "SD", "1HE", "OH", "2HE",
              "CZ", "HZ", "NE", "HE")
TILE_SIZES = (1, 7, 8, 9, 16, 17, 24)
TILE_CORNERS = ("first_first", "first_last", "last_first", "last_last")
STEP = np.array([300, 400, 0], dtype=np.int64)              # length 500
REACH = np.array([3000, 4000, 0], dtype=np.int64)           # length 5000


def anchors(at):
    """A receptor residue and a ligand residue of N, CA, C, O each, 8 A apart: fit atoms and an interface for complexes whose
    residues under test have too few; no native pair at C <= 7000."""
    at = np.asarray(at, dtype=np.int64)
    quad = np.array([[0, 0, 0], [1458, 0, 0], [2009, 1420, 0], [1600, 2100, 950]], dtype=np.int64)
    rec = [atom(FIT_CYCLE[i], "GLY", "A", 900, at + q) for i, q in enumerate(quad)]
    lig = [atom(FIT_CYCLE[i], "GLY", "B", 900, at + q + np.array([0, 0, 9000])) for i, q in enumerate(quad)]
    return rec, lig


def tile_residues(n_rec, n_lig, corner, at=(20000, 20000, 20000), seq=1, reach=REACH):
    """A receptor residue of n_rec atoms and a ligand residue of n_lig: the contacting atoms `reach` apart, first or last of
    their residue; atom k of the others another 0.5 A a step further from the other residue, along `reach`'s direction."""
    at = np.asarray(at, dtype=np.int64)
    a_place, b_place = corner.split("_")
    step = np.asarray(reach) // 10
    rec_pts = [at - k * step for k in range(n_rec)]
    lig_pts = [at + reach + k * step for k in range(n_lig)]
    if a_place == "last":
        rec_pts = rec_pts[1:] + rec_pts[:1]
    if b_place == "last":
        lig_pts = lig_pts[1:] + lig_pts[:1]
    rec = [atom(FILL_NAMES[k], "LYS", "A", seq, p) for k, p in enumerate(rec_pts)]
    lig = [atom(FILL_NAMES[k], "ARG", "B", seq, p) for k, p in enumerate(lig_pts)]
    return rec, lig


def noisy(atoms, seed):
    """The same records a little elsewhere, so that no RMSD is 0."""
    rng = np.random.default_rng(seed)
    return [atom(a[0], a[1], a[2], a[3], np.array(a[4]) + rng.integers(-300, 301, size=3)) for a in atoms]


@functools.lru_cache(maxsize=None)
def tile_case(n_rec, n_lig, corner, poses=((0, 0, 0), (1, 0, 0))):
    """One native pair whose only contacting atom pair is 3000, 4000, 0 apart (exactly C = 5000) at pose 0 and 3001, 4000, 0 at
    pose 1; every other atom pair of the two residues at 5500 at least.  The reference holds the pair in contact (the model's
    records at pose 0) and the anchors a little elsewhere."""
    rec, lig = tile_residues(n_rec, n_lig, corner)
    arec, alig = anchors((60000, 20000, 20000))
    return Case("tile_%d_%d_%s" % (n_rec, n_lig, corner), rec + arec, lig + alig, rec + noisy(arec, 1), lig + noisy(alig, 2), poses=poses,
                tile=(n_rec, n_lig, corner))


def tile_cases(corner):
    return [tile_case(a, b, corner) for a in TILE_SIZES for b in TILE_SIZES]


PAIR_COUNTS = (1, 7, 8, 9, 17)
PAIR_POSES = ((0, 0, 0), (0, 1, 0), (1, 0, 0), (-1, 0, 0))     # all kept; none; the even pairs; the odd pairs


@functools.lru_cache(maxsize=None)
def pairs_case(count):
    """`count` native pairs 100 A apart, pair i's contact 3000, 4000, 0 apart for odd i and -3000, 4000, 0 for even i: a step of
    the ligand in +x keeps the even pairs only, in -x the odd ones, in +y none.  8 waves take the pairs in turn."""
    rec, lig = [], []
    for i in range(count):
        reach = REACH * np.array([1 if i % 2 else -1, 1, 1])
        r, l = tile_residues(3, 2, "first_first", (20000, 20000, 20000 + 100000 * i), i + 1, reach)
        rec, lig = rec + r, lig + l
    arec, alig = anchors((60000, 20000, 20000))
    kept = [count, 0, (count + 1) // 2, count // 2]
    return Case("pairs_%d" % count, rec + arec, lig + alig, rec + noisy(arec, 3), lig + noisy(alig, 4), poses=PAIR_POSES, kept=kept)


CUTOFF_POSES = ((0, 0, 0), (0, 1, 0), (1, 0, 0), (-1, 0, 0))   # C, 0, 0: in; C, 1, 0: out; C + 1, 0, 0: out; C - 1, 0, 0: in


@functools.lru_cache(maxsize=None)
def cutoff_case(C):
    """C = 1 and C = 30000: the pair's atoms C apart along x."""
    at = np.array([20000, 20000, 20000], dtype=np.int64)
    rec = [atom("CA", "LYS", "A", 1, at), atom("CB", "LYS", "A", 1, at - (40000, 0, 0))]
    lig = [atom("CA", "ARG", "B", 1, at + (C, 0, 0)), atom("CB", "ARG", "B", 1, at + (C + 40000, 0, 0))]
    arec, alig = anchors((20000, 90000, 20000))
    return Case("cutoff_%d" % C, rec + arec, lig + alig, rec + noisy(arec, 5), lig + noisy(alig, 6), poses=CUTOFF_POSES, C=C,
                I=max(C, 10000), kept_of_pair=[1, 0, 0, 1])


def aliasing_distances(limit, lo=65536, hi=3998000):
    """Every d in [lo, hi] with d^2 mod 2^32 <= limit (hi: the ligand's other atom, 1.1 A further, stays within 2000 A)."""
    d = np.arange(lo, hi + 1, dtype=np.uint64)
    return d[(d * d) % np.uint64(2 ** 32) <= np.uint64(limit)].astype(np.int64)


@functools.lru_cache(maxsize=None)
def aliases():
    """(distances on x alone: the smallest, one in the middle, the largest; a triple for the three axes at once whose squares'
    32-bit sum is under C^2 as well)."""
    C2 = 5000 * 5000
    single = aliasing_distances(limit=C2)
    third = aliasing_distances(limit=C2 // 3)
    return [int(single[0]), int(single[len(single) // 2]), int(single[-1])], tuple(int(v) for v in (third[0], third[len(third) // 2], third[-1]))


@functools.lru_cache(maxsize=None)
def aliasing_case():
    """One native pair; the receptor's atom at -1999.9 A on every axis, the ligand's posed d thousandths from it on x alone, or
    d_x, d_y, d_z on all three.  A distance test in unclamped 32-bit arithmetic would call each of them a contact."""
    single, triple = aliases()
    at = np.array([-1999900, -1999900, -1999900], dtype=np.int64)
    home = np.array([20000, 20000, 20000], dtype=np.int64)
    rec = [atom("CA", "LYS", "A", 1, at), atom("N", "LYS", "A", 1, at + (1300, 500, 0)), atom("C", "LYS", "A", 1, at + (200, 1400, 700))]
    lig = [atom("CA", "ARG", "B", 1, home), atom("N", "ARG", "B", 1, home + (900, 1100, 300))]
    ref_at = np.array([30000, 30000, 30000], dtype=np.int64)
    ref_rec = with_xyz(rec, [ref_at, ref_at + (1300, 500, 0), ref_at + (200, 1400, 700)])
    ref_lig = with_xyz(lig, [ref_at + (3000, 0, 0), ref_at + (3900, 1100, 300)])
    poses = [tuple(at - home + (3000, 0, 0))] + [tuple(at - home + (d, 0, 0)) for d in single] + [tuple(at - home + triple)]
    return Case("aliasing", rec, lig, ref_rec, ref_lig, poses=poses, kept=[1, 0, 0, 0, 0], distances=(single, triple))


USED_COUNTS = ((3, 1), (63, 64), (64, 513), (65, 1), (511, 64), (512, 513), (513, 1))


def grid(k, origin):
    return np.asarray(origin, dtype=np.int64) + 4000 * np.array([k % 8, (k // 8) % 8, k // 64], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def used_case(n_rec_used, n_lig_used):
    """Exactly n_rec_used and n_lig_used used atoms, the five kinds of atom interleaved in file order: unmatched (absent from the
    reference), matched but unused, used but no fit atom, fit atoms outside the interface, interface fit atoms."""
    centre = np.array([200000, 200000, 200000], dtype=np.int64)
    rec, lig, absent = [], [], set()

    def filler(chain, seq, p, order):
        made = {"fit": atom(FIT_CYCLE[seq % 5], "VAL", chain, seq, p), "unused": atom("CB", "VAL", chain, seq, p + (1500, 0, 0)),
                "absent": atom("HX", "VAL", chain, seq, p + (0, 1000, 0))}
        absent.add((chain, seq, "HX"))
        return [made[k] for k in order]

    orders = (("fit", "unused", "absent"), ("absent", "fit", "unused"), ("unused", "absent", "fit"))
    n_fill = max(0, n_rec_used - 4)
    native_rec = [atom("N", "LYS", "A", 5000, centre), atom("HZ", "LYS", "A", 5000, centre + (0, 900, 0)),
                  atom("CA", "LYS", "A", 5000, centre + (1400, 300, 0)),
                  atom("C" if n_rec_used == 3 else "CB", "LYS", "A", 5000, centre + (1900, 1500, 800))]
    absent.add(("A", 5000, "HZ"))
    near_rec = [atom("CA", "THR", "A", 5001, centre + (-7000, 0, 0)), atom("CG", "THR", "A", 5001, centre + (-8000, 1000, 0))]
    if n_rec_used == 3:
        near_rec = []
    for k in range(n_fill):
        if k == n_fill // 2:
            rec += native_rec + near_rec
        rec += filler("A", k + 1, grid(k, (100000, 100000, 100000)), orders[k % 3])
    if n_fill == 0:
        rec += native_rec + near_rec
    native_lig = ([atom("HZ", "ARG", "B", 5000, centre + (0, 3900, 0)), atom("CA", "ARG", "B", 5000, centre + (0, 3000, 0))] +
                  ([] if n_lig_used == 1 else [atom("CB", "ARG", "B", 5000, centre + (0, 4000, 1200))]))
    absent.add(("B", 5000, "HZ"))
    n_fill = max(0, n_lig_used - 2)
    for k in range(n_fill):
        if k == n_fill // 3:
            lig += native_lig
        lig += filler("B", k + 1, grid(k, (300000, 300000, 300000)), orders[(k + 1) % 3])
    if n_fill == 0:
        lig += native_lig
    keep = lambda atoms: [a for a in atoms if (a[2], a[3], a[0]) not in absent]
    return Case("used_%d_%d" % (n_rec_used, n_lig_used), noisy(rec, 7), noisy(lig, 8), keep(rec), keep(lig), poses=((0, 0, 0), (150, -90, 60)),
                used=(n_rec_used, n_lig_used))


BOUND_POSES = ((1990000, 0, 0), (-2006000, 0, 0), (0, 1990000, 0), (0, 0, -2006000), (0, 0, 0))
REFUSED_ROWS = np.array([[1990.0006, 0, 0, 1, 0, 0, 0.0], [0, -2006.0006, 0, 1, 0, 0, 0.0], [0, 0, 1990.001, 1, 0, 0, 0.0]])
ACCEPTED_ROWS = np.array([[1990.0004, 0, 0, 1, 0, 0, 0.0], [0, 0, -2006.0004, 1, 0, 0, 0.0]])       # print as +-2000.000


@functools.lru_cache(maxsize=None)
def bound_case():
    """The ligand's used atoms span 6.000 .. 10.000 A on every axis: a translation by 1990 A puts one at exactly 2000.000 A, by
    -2006 A one at -2000.000 A.  An unmatched ligand atom sits at 5000 A and a matched but unused one at 4000 A in the file."""
    rec, lig = tile_residues(3, 2, "first_first", (3000, 2000, 8000))       # the ligand's two atoms at 6000, 6000, 8000 and 6300, 6400, 8000
    lig = lig + [atom("CA", "GLY", "B", 2, (10000, 10000, 10000)), atom("N", "GLY", "B", 2, (6000, 10000, 6000)),
                 atom("HX", "GLY", "B", 2, (5000000, 5000000, 5000000)), atom("CB", "GLY", "B", 2, (4000000, 4000000, 4000000))]
    rec = rec + [atom("O", "GLY", "A", 2, (1000, 5000, 9000))]              # off the line of the other three
    ref_lig = [a for a in lig if a[0] != "HX"]
    ref_lig = [atom(a[0], a[1], a[2], a[3], (9000, 9000, 9000)) if a[0] == "CB" and a[3] == 2 else a for a in ref_lig]
    return Case("bound", rec, lig, noisy(rec, 9), ref_lig, poses=BOUND_POSES, bound=True)


def slot_case():
    """The last lane of the last tile, 1030 poses that alternate between in and out: more poses than slots."""
    return tile_case(17, 9, "last_last", poses=tuple((k % 2, 0, 0) for k in range(1030)))


def sums_cases():
    cases = [tile_case(a, b, corner) for corner in TILE_CORNERS for a in TILE_SIZES for b in TILE_SIZES]
    cases += [pairs_case(n) for n in PAIR_COUNTS] + [cutoff_case(1), cutoff_case(30000), aliasing_case()]
    return cases + [used_case(a, b) for a, b in USED_COUNTS] + [bound_case(), slot_case()]


def all_cases():
    return solver_cases() + [spread_case()] + sums_cases()
