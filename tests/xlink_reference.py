"""The cross-link rule of include/lightdock_hip.h ("Cross-links") restated in integer numpy, from the text:
the checker of tests/test_xlink_cpu.py and tests/test_gpu_xlink.py.  Shortest paths on the lattice (i h, j h, k h) over the
nodes no blocker holds strictly inside its expanded sphere, 26 moves of weights h, isqrt(2 h^2), isqrt(3 h^2), a hop of
isqrt(|q - c|^2) between an anchor and each of its doors.  Posing, rounding and radii are SasaRestated's
(tests/sasa_reference.py), the exact square root is ccs_reference's.

Blocked nodes: every blocker against every node of its own bounding cube inside the box, the rule's inequality itself.
The field of a source anchor: all of the box relaxed over the 26 shifts, again and again, until nothing changes -- no
levels, no queue, no sub-box, so a disagreement with the kernel's schedule would show."""
import math
import os

import numpy as np

import sasa_reference as sr
from ccs_reference import ceil_div, isqrt
from sasa_reference import thousandths  # noqa: F401

NO_PATH = 0xFFFFFFFF
COORD_BOUND = 10 ** 9
MAX_LINKS = 4096
BIG = 1 << 30
SHIFTS = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]


class Refused(Exception):
    """What the rule refuses with LD_ERR_INVALID."""


def parameters(probe=0.0, cell=1.0, reach=3.0, max_length=35.0):
    """-> (p, h, rho, M) in thousandths, or Refused."""
    for v in (probe, cell, reach, max_length):
        if not math.isfinite(v) or abs(v) > 1e6:
            raise Refused("a parameter is not finite")
    p, h, rho, M = (int(round(1000.0 * v)) for v in (probe, cell, reach, max_length))
    if not (0 <= p <= 2000 and 500 <= h <= 2000 and 1 <= rho <= 6000 and h <= M <= 60000 and M // h <= 80):
        raise Refused("a parameter is out of range")
    return p, h, rho, M


def weights(h):
    return h, math.isqrt(2 * h * h), math.isqrt(3 * h * h)


def straight2(t, links):
    """|c_a - c_b|^2 of every link as Python integers."""
    return [sum(int(v) ** 2 for v in (t[a] - t[b])) for a, b in links]


def box_of(c, M, h):
    """(lo (3,), n (3,)): on every axis the nodes lo .. lo + n - 1 within M of c."""
    lo = np.array([ceil_div(int(v) - M, h) for v in c], dtype=np.int64)
    hi = np.array([(int(v) + M) // h for v in c], dtype=np.int64)
    return lo, hi - lo + 1


def axes(lo, n, h):
    return [(lo[k] + np.arange(n[k], dtype=np.int64)) * h for k in range(3)]


def squared_distance(lo, n, h, c):
    """|q - c|^2 of every node of the box, (nx, ny, nz) int64."""
    x, y, z = axes(lo, n, h)
    return ((x - int(c[0])) ** 2)[:, None, None] + ((y - int(c[1])) ** 2)[None, :, None] + ((z - int(c[2])) ** 2)[None, None, :]


def blocked_nodes(lo, n, h, bc, bE):
    """bool (nx, ny, nz): node q is blocked iff some blocker x has |q - c_x|^2 < E_x^2."""
    out = np.zeros(tuple(n), dtype=bool)
    for c, E in zip(bc, bE):
        E = int(E)
        a = [max(ceil_div(int(c[k]) - E, h), int(lo[k])) for k in range(3)]
        b = [min((int(c[k]) + E) // h, int(lo[k] + n[k] - 1)) for k in range(3)]
        if any(a[k] > b[k] for k in range(3)):
            continue
        sub_lo, sub_n = np.array(a, dtype=np.int64), np.array([b[k] - a[k] + 1 for k in range(3)], dtype=np.int64)
        s = tuple(slice(a[k] - int(lo[k]), b[k] - int(lo[k]) + 1) for k in range(3))
        out[s] |= squared_distance(sub_lo, sub_n, h, c) < E * E
    return out


def doors(lo, n, h, c, rho, blocked):
    """(mask (nx, ny, nz) of the free nodes within rho of c, their hops isqrt(|q - c|^2) (same shape, int64))."""
    d2 = squared_distance(lo, n, h, c)
    return (d2 <= rho * rho) & ~blocked, isqrt(d2)


def field(blocked, door, hop, h):
    """The shortest distance of every node of the box from the anchor through its doors, int64 (nx, ny, nz), BIG where
    there is none: relaxed over the 26 shifts until nothing changes."""
    shape = blocked.shape
    D = np.full(tuple(s + 2 for s in shape), BIG, dtype=np.int32)
    inner = D[1:-1, 1:-1, 1:-1]
    inner[door] = hop[door]
    hold = np.where(blocked, BIG, 0).astype(np.int32)        # a blocked node stays where it is
    w = weights(h)
    tmp = np.empty(shape, dtype=np.int32)
    while True:
        before = inner.copy()
        for dx, dy, dz in SHIFTS:
            src = D[1 + dx:1 + dx + shape[0], 1 + dy:1 + dy + shape[1], 1 + dz:1 + dz + shape[2]]
            np.add(src, w[abs(dx) + abs(dy) + abs(dz) - 1], out=tmp)
            np.maximum(tmp, hold, out=tmp)
            np.minimum(inner, tmp, out=inner)
        if np.array_equal(before, inner):
            return inner.astype(np.int64)


def path_lengths(t, radii, links, probe=0.0, cell=1.0, reach=3.0, max_length=35.0, cache=None):
    """t (atoms, 3) int64 thousandths of a posed complex, radii (atoms,) with 0 for an atom that takes no part, links
    (L, 2) -> (L,) int64: D, or NO_PATH.  The source of a link is its first anchor; `cache` keeps a source's field."""
    p, h, rho, M = parameters(probe, cell, reach, max_length)
    t, radii = np.asarray(t, dtype=np.int64), np.asarray(radii, dtype=np.int64)
    part = np.flatnonzero(radii > 0)
    if len(part) == 0:
        raise Refused("no atom takes part")
    anchors = sorted({int(v) for v in np.asarray(links).ravel()})
    if np.abs(t[part]).max() > COORD_BOUND or np.abs(t[anchors]).max() > COORD_BOUND:
        raise Refused("a posed blocker or anchor is beyond +-1.0e6 A")
    bc, bE = t[part], radii[part] + p
    cache = {} if cache is None else cache
    out = []
    for a, b in links:
        a, b = int(a), int(b)
        if a not in cache:
            lo, n = box_of(t[a], M, h)
            blocked = blocked_nodes(lo, n, h, bc, bE)
            door, hop = doors(lo, n, h, t[a], rho, blocked)
            cache[a] = (lo, n, blocked, field(blocked, door, hop, h))
        lo, n, blocked, D = cache[a]
        door, hop = doors(lo, n, h, t[b], rho, blocked)
        total = (D + hop)[door & (D < BIG)]
        best = int(total.min()) if total.size else NO_PATH
        out.append(best if best <= M else NO_PATH)
    return np.array(out, dtype=np.int64)


def check_links(links, n_atoms):
    links = np.asarray(links, dtype=np.int64).reshape(-1, 2)
    if not 1 <= len(links) <= MAX_LINKS or (links < 0).any() or (links >= n_atoms).any():
        raise Refused("links")
    return links


class XlinkRestated(sr.SasaRestated):
    def crosslinks(self, row, links, probe=0.0, cell=1.0, reach=3.0, max_length=35.0, paths=True):
        """One pose -> (straight2: L Python integers, path: (L,) int64 or None)."""
        parameters(probe, cell, reach, max_length)
        links = check_links(links, len(self.radii))
        t = thousandths(self.pose(row))
        if np.abs(t[np.unique(links)]).max() > COORD_BOUND:
            raise Refused("a posed anchor is beyond +-1.0e6 A")
        return straight2(t, links), (path_lengths(t, self.radii, links, probe, cell, reach, max_length) if paths else None)

    def batch(self, poses, links, probe=0.0, cell=1.0, reach=3.0, max_length=35.0):
        """-> (straight2 (n, L) uint64, path (n, L) uint32)."""
        got = [self.crosslinks(p, links, probe, cell, reach, max_length) for p in poses]
        L = len(np.asarray(links).reshape(-1, 2))
        return (np.array([g[0] for g in got], dtype=np.uint64).reshape(len(got), L),
                np.array([g[1] for g in got], dtype=np.uint32).reshape(len(got), L))


def czy_xlink(modes=True):
    from test_analysis_cpu import CZY
    rec, lig = os.path.join(CZY, "lightdock_1czy_protein.pdb"), os.path.join(CZY, "lightdock_1czy_peptide.pdb")
    if not modes:
        return XlinkRestated(rec, lig)
    return XlinkRestated(rec, lig, np.load(os.path.join(CZY, "lightdock_rec.nm.npy")), np.load(os.path.join(CZY, "lightdock_lig.nm.npy")))
