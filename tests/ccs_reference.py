"""The collision cross-section rule of include/lightdock_hip.h ("Collision cross-section") restated in int64
numpy, from the text: the checker of tests/test_ccs_cpu.py and tests/test_gpu_ccs.py.  The projection approximation on the
thousandths "%8.3f" prints: 64 fixed integer frames, expanded radii E = R + p, the lattice (i h, j h) of every view, a point
covered by atom a iff (i h - a)^2 + (j h - b)^2 <= E^2.  Posing, rounding and radii are SasaRestated's (tests/sasa_reference.py).

The covered points of a view are held as a sparse set built atom by atom: for every atom and every lattice row its disc
touches, the interval of columns that satisfy the inequality; the set is the union of the intervals row by row, and its size
the count.  Nothing is allocated over a box, so a huge box costs nothing."""
import math
import os

import numpy as np

import sasa_reference as sr
from sasa_reference import thousandths  # noqa: F401

VIEWS = 64
MAX_BOX = 1 << 28
COORD_BOUND = 10 ** 9


class Refused(Exception):
    """What the rule refuses with LD_ERR_INVALID."""


def frames(margin=False):
    """(64, 2, 3) int64: A[v] = rint(2^20 e1), B[v] = rint(2^20 e2), e1 = (-s, c, 0), e2 = (-z c, -z s, r), z = 1 - (2v + 1) / 128,
    r = sqrt(1 - z^2), c = cos(v g), s = sin(v g), g = pi (3 - sqrt 5).  margin=True: also the least distance of a scaled
    component from a rounding tie."""
    v = np.arange(VIEWS, dtype=np.float64)
    z = 1.0 - (2.0 * v + 1.0) / 128.0
    r = np.sqrt(1.0 - z * z)
    g = math.pi * (3.0 - math.sqrt(5.0))
    c, s = np.cos(v * g), np.sin(v * g)
    scaled = 2.0 ** 20 * np.stack([np.stack([-s, c, np.zeros(VIEWS)], axis=1), np.stack([-z * c, -z * s, r], axis=1)], axis=1)
    table = np.rint(scaled).astype(np.int64)
    if margin:
        return table, float(np.abs(np.abs(scaled - np.floor(scaled)) - 0.5).min())
    return table


FRAMES = frames()


def project(t):
    """t (atoms, 3) int64 thousandths -> (a, b), each (64, atoms): (F . c + 2^19) >> 20, the shift arithmetic."""
    t = np.asarray(t, dtype=np.int64)
    a = (FRAMES[:, 0, :] @ t.T + (1 << 19)) >> 20
    b = (FRAMES[:, 1, :] @ t.T + (1 << 19)) >> 20
    return a, b


def isqrt(v):
    """floor(sqrt(v)) of an int64 array of values >= 0, exactly."""
    w = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
    w -= w * w > v
    w += (w + 1) * (w + 1) <= v
    assert ((w * w <= v) & ((w + 1) * (w + 1) > v)).all()
    return w


def ceil_div(x, h):
    return -((-x) // h)


def box_points(a, b, E, h):
    """I x J: the lattice columns and rows that the box [min(a - E), max(a + E)] x [min(b - E), max(b + E)] touches."""
    I = int((a + E).max()) // h - ceil_div(int((a - E).min()), h) + 1
    J = int((b + E).max()) // h - ceil_div(int((b - E).min()), h) + 1
    return I * J


def spans(a, b, E, h):
    """The sparse set of one view: (j, lo, hi) of every atom and every lattice row its disc touches with a covered column:
    lo .. hi are the columns i with (i h - a)^2 <= E^2 - (j h - b)^2."""
    j_lo, j_hi = ceil_div(b - E, h), (b + E) // h
    n = j_hi - j_lo + 1
    assert (n >= 1).all()
    atom = np.repeat(np.arange(len(a)), n)
    j = np.repeat(j_lo, n) + np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    dy = j * h - b[atom]
    v = E[atom] * E[atom] - dy * dy
    assert (v >= 0).all()
    w = isqrt(v)
    lo, hi = ceil_div(a[atom] - w, h), (a[atom] + w) // h
    keep = lo <= hi
    return j[keep], lo[keep], hi[keep]


def union_size(j, lo, hi):
    """The number of points of the union of the intervals (j, lo .. hi)."""
    if len(j) == 0:
        return 0
    big = int(hi.max() - lo.min()) + 4
    lo_key, hi_key = j * big + (lo - lo.min() + 1), j * big + (hi - lo.min() + 1)        # rows apart: a row's keys never meet the next's
    order = np.argsort(lo_key, kind="stable")
    lo_key, hi_key = lo_key[order], hi_key[order]
    reach = np.maximum.accumulate(hi_key)
    before = np.concatenate([[lo_key[0] - 1], reach[:-1]])
    return int(np.maximum(0, hi_key - np.maximum(before, lo_key - 1)).sum())


def view_count(a, b, E, h):
    return union_size(*spans(a, b, E, h))


def counts(t, E, h):
    """t (atoms, 3) int64 thousandths, E (atoms,) expanded radii, the step h -> (64,) covered lattice points of every view.
    Refused: a coordinate beyond +-1.0e6 A, a view's box of more than 2^28 points."""
    t, E = np.asarray(t, dtype=np.int64), np.asarray(E, dtype=np.int64)
    if len(t) == 0:
        raise Refused("no selected atom takes part")
    if np.abs(t).max() > COORD_BOUND:
        raise Refused("a posed coordinate is beyond +-1.0e6 A")
    a, b = project(t)
    if max(box_points(a[v], b[v], E, h) for v in range(VIEWS)) > MAX_BOX:
        raise Refused("a view's box holds more than 2^28 lattice points")
    return np.array([view_count(a[v], b[v], E, h) for v in range(VIEWS)], dtype=np.int64)


def brute_count(a, b, E, h):
    """The rule's inequality on every lattice point of the atoms' box, one view: only for small boxes."""
    i = np.arange(ceil_div(int((a - E).min()), h), int((a + E).max()) // h + 1, dtype=np.int64)
    j = np.arange(ceil_div(int((b - E).min()), h), int((b + E).max()) // h + 1, dtype=np.int64)
    covered = np.zeros((len(i), len(j)), dtype=bool)
    for x, y, e in zip(a, b, E):
        covered |= ((i * h - x) ** 2)[:, None] + ((j * h - y) ** 2)[None, :] <= e * e
    return int(covered.sum())


def step(cell):
    h = int(round(1000.0 * cell))
    if not 100 <= h <= 2000:
        raise Refused("cell out of range")
    return h


def area(points, cell=0.5):
    """Covered points of a view -> A^2."""
    h = step(cell)
    return np.asarray(points, dtype=np.float64) * float(h * h) / 1e6


def ccs_pa(sums, cell=0.5):
    """sums (over the 64 views) -> CCS_PA in A^2."""
    return area(sums, cell) / VIEWS


class CcsRestated(sr.SasaRestated):
    def selected(self, what):
        if what not in (0, 1, 2):
            raise Refused("what")
        part = self.radii > 0
        side = np.arange(len(self.radii)) >= self.n_rec
        return np.flatnonzero(part & {0: ~side, 1: side, 2: np.ones_like(side)}[what])

    def of_xyz(self, xyz, what=2, probe=1.0, cell=0.5):
        sel = self.selected(what)
        return counts(thousandths(xyz)[sel], self.radii[sel] + sr.probe_thousandths(probe), step(cell))

    def ccs(self, row, what=2, probe=1.0, cell=0.5):
        """One pose -> (64,) int64 counts."""
        return self.of_xyz(self.pose(row), what, probe, cell)

    def batch(self, poses, what=2, probe=1.0, cell=0.5):
        """-> (counts (n, 64) uint32, sums (n,) uint64)."""
        got = np.array([self.ccs(p, what, probe, cell) for p in poses], dtype=np.int64).reshape(len(poses), VIEWS)
        return got.astype(np.uint32), got.sum(axis=1).astype(np.uint64)


def czy_ccs(modes=True):
    from test_analysis_cpu import CZY
    rec, lig = os.path.join(CZY, "lightdock_1czy_protein.pdb"), os.path.join(CZY, "lightdock_1czy_peptide.pdb")
    if not modes:
        return CcsRestated(rec, lig)
    return CcsRestated(rec, lig, np.load(os.path.join(CZY, "lightdock_rec.nm.npy")), np.load(os.path.join(CZY, "lightdock_lig.nm.npy")))
