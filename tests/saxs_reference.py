"""The small-angle scattering rule of include/lightdock_hip.h ("Small-angle scattering") restated in numpy,
from the text: the checker of tests/test_saxs_cpu.py and tests/test_gpu_saxs.py.  The pair-distance histogram by pair class
is int64 on the thousandths "%8.3f" prints; the tables come from math.exp / math.sin; the Debye sums are a Python loop
over k on arrays, so that every sum has the rule's order.  Posing and rounding are ContactsRestated's
(tests/test_contacts_cpu.py), the element is sasa_reference's."""
import math
import os

import numpy as np

from sasa_reference import element, records
from test_contacts_cpu import ContactsRestated, thousandths

CLASSES, PAIR_CLASSES = 6, 21
NO_PART = 255
CLASS_OF = {"H": 0, "D": 0, "C": 1, "N": 2, "O": 3, "P": 4, "S": 5}
RHO0 = 0.334
AXIS_CLAMP = 2 ** 22 - 1
# a1..a4, b1..b4, c, V of H, C, N, O, P, S
TABLE = (
    ((0.489918, 0.262003, 0.196767, 0.049879), (20.6593, 7.74039, 49.5519, 2.20159), 0.001305, 5.15),
    ((2.31000, 1.02000, 1.58860, 0.865000), (20.8439, 10.2075, 0.568700, 51.6512), 0.215600, 16.44),
    ((12.2126, 3.13220, 2.01250, 1.16630), (0.005700, 9.89330, 28.9975, 0.582600), -11.529, 2.49),
    ((3.04850, 2.28680, 1.54630, 0.867000), (13.2771, 5.70110, 0.323900, 32.9089), 0.250800, 9.13),
    ((6.43450, 4.17910, 1.78000, 1.49080), (1.90670, 27.1570, 0.526000, 68.1645), 1.11490, 5.73),
    ((6.90530, 5.20340, 1.43790, 1.58630), (1.46790, 22.2151, 0.253600, 56.1720), 0.866900, 19.86),
)
Z = (1, 6, 7, 8, 15, 16)


def pair_class(e, f):
    lo, hi = min(e, f), max(e, f)
    return 6 * lo - lo * (lo - 1) // 2 + (hi - lo)


PAIRS = [(e, f) for e in range(CLASSES) for f in range(e, CLASSES)]     # PAIRS[c] = (e, e')
assert [pair_class(e, f) for e, f in PAIRS] == list(range(PAIR_CLASSES))


def record_class(record):
    if record[17:20].strip() == "MMB":
        return NO_PART
    return CLASS_OF.get(element(record), NO_PART)


def file_classes(path):
    return np.array([record_class(r) for r in records(path)], dtype=np.int64)


def form_factor(e, q):
    a, b, c, V = TABLE[e]
    u = (q / (4.0 * math.pi)) ** 2
    return sum(ak * math.exp(-bk * u) for ak, bk in zip(a, b)) + c - RHO0 * V * math.exp(-q * q * V ** (2.0 / 3.0) / (4.0 * math.pi))


def form_factors(q):
    return np.array([[form_factor(e, float(x)) for e in range(CLASSES)] for x in q]).reshape(len(q), CLASSES)


def sinc(q, w, bins):
    """(n_q, bins): s(q_j r_k), r_k = (k + 0.5) w / 1000."""
    out = np.zeros((len(q), bins))
    for j, x in enumerate(q):
        for k in range(bins):
            v = float(x) * ((k + 0.5) * w / 1000.0)
            out[j, k] = 1.0 if v == 0.0 else math.sin(v) / v
    return out


def isqrt(d2):
    """floor(sqrt(d2)) of an int64 array, exactly."""
    s = np.floor(np.sqrt(d2.astype(np.float64))).astype(np.int64)
    s -= (s * s > d2)
    s += ((s + 1) * (s + 1) <= d2)
    return s


def histogram(t, classes, w, bins):
    """t: (atoms, 3) int64 thousandths of a posed complex; classes: (atoms,), 255 = takes no part -> (21, bins) int64.
    ValueError when a pair lies beyond the last bin."""
    part = np.flatnonzero(np.asarray(classes) != NO_PART)
    c, e = np.asarray(t, dtype=np.int64)[part], np.asarray(classes, dtype=np.int64)[part]
    out = np.zeros(PAIR_CLASSES * bins, dtype=np.int64)
    a, b = np.triu_indices(len(part), 1)
    if len(a):
        d = np.minimum(np.abs(c[a] - c[b]), AXIS_CLAMP)
        k = isqrt((d * d).sum(axis=1)) // w                      # the largest k with (k w)^2 <= d^2
        if (k >= bins).any():
            raise ValueError("a pair lies beyond the last bin")
        lo, hi = np.minimum(e[a], e[b]), np.maximum(e[a], e[b])
        out += np.bincount((6 * lo - lo * (lo - 1) // 2 + (hi - lo)) * bins + k, minlength=PAIR_CLASSES * bins)
    return out.reshape(PAIR_CLASSES, bins)


def class_atoms(classes):
    return np.array([int((np.asarray(classes) == e).sum()) for e in range(CLASSES)], dtype=np.int64)


def debye(counts, n_e, f, s):
    """counts (21, bins), n_e (6,), f (n_q, 6), s (n_q, bins) -> I (n_q,), every sum in the rule's order."""
    counts = np.asarray(counts)
    n_q, bins = s.shape
    G = np.zeros((n_q, PAIR_CLASSES))
    for k in range(bins):                                        # k ascending, from 0
        G = G + counts[:, k].astype(np.float64)[None, :] * s[:, k][:, None]
    S = np.zeros(n_q)
    for e in range(CLASSES):
        S = S + float(n_e[e]) * (f[:, e] * f[:, e])
    out = S
    for c, (e, g) in enumerate(PAIRS):
        out = out + ((2.0 * f[:, e]) * f[:, g]) * G[:, c]
    return out


def fit(I, i_exp, sigma):
    """One pose: sequential Python sums -> (scale, chi2)."""
    num = den = 0.0
    for j in range(len(i_exp)):
        s2 = float(sigma[j]) * float(sigma[j])
        num = num + float(i_exp[j]) * float(I[j]) / s2
        den = den + float(I[j]) * float(I[j]) / s2
    scale = num / den
    total = 0.0
    for j in range(len(i_exp)):
        r = (float(i_exp[j]) - scale * float(I[j])) / float(sigma[j])
        total = total + r * r
    return scale, total / len(i_exp)


def direct(t, classes, q):
    """The unbinned Debye sum over atom pairs -> (I (n_q,), sum over a < b of |f_a f_b| (n_q,))."""
    part = np.flatnonzero(np.asarray(classes) != NO_PART)
    c, e = np.asarray(t, dtype=np.int64)[part], np.asarray(classes, dtype=np.int64)[part]
    a, b = np.triu_indices(len(part), 1)
    d = c[a] - c[b]
    r = np.sqrt((d * d).sum(axis=1).astype(np.float64)) / 1000.0
    f = form_factors(q)
    out, weight = np.zeros(len(q)), np.zeros(len(q))
    for j, x in enumerate(q):
        fa = f[j][e]
        ff = fa[a] * fa[b]
        out[j] = (fa * fa).sum() + 2.0 * (ff * np.sinc(float(x) * r / math.pi)).sum()
        weight[j] = np.abs(ff).sum()
    return out, weight


class SaxsRestated(ContactsRestated):
    def __init__(self, rec_pdb, lig_pdb, rec_modes=None, lig_modes=None):
        ContactsRestated.__init__(self, rec_pdb, lig_pdb, rec_modes, lig_modes)
        self.classes = np.concatenate([file_classes(rec_pdb), file_classes(lig_pdb)])
        self.n_e = class_atoms(self.classes)
        self.n_part = int(self.n_e.sum())

    def thousandths(self, row):
        return thousandths(self.pose(row))

    def counts(self, row, w=500, bins=1024):
        return histogram(self.thousandths(row), self.classes, w, bins)

    def batch(self, poses, w=500, bins=1024):
        return np.array([self.counts(p, w, bins) for p in poses], dtype=np.uint32).reshape(len(poses), PAIR_CLASSES, bins)

    def profile(self, counts, f, s):
        return debye(counts, self.n_e, f, s)


def czy_saxs():
    from test_analysis_cpu import CZY
    return SaxsRestated(os.path.join(CZY, "lightdock_1czy_protein.pdb"), os.path.join(CZY, "lightdock_1czy_peptide.pdb"),
                        np.load(os.path.join(CZY, "lightdock_rec.nm.npy")), np.load(os.path.join(CZY, "lightdock_lig.nm.npy")))
