"""The solvent-accessible surface rule of include/lightdock_hip.h ("Solvent-accessible surface") restated in
int64 numpy, from the text: the checker of tests/test_sasa_cpu.py and tests/test_gpu_sasa.py.  Shrake-Rupley on the
thousandths "%8.3f" prints: 128 fixed integer directions, expanded radii E = R + p, a point q of atom a is buried by atom
b != a iff |q - c_b|^2 < E_b^2.  Posing and rounding are ContactsRestated's (tests/test_contacts_cpu.py)."""
import math
import os

import numpy as np

from test_contacts_cpu import ContactsRestated, case_restated, thousandths  # noqa: F401

POINTS = 128
RADII = {"C": 1700, "N": 1550, "O": 1520, "F": 1470, "P": 1800, "S": 1800, "CL": 1750, "SE": 1900, "BR": 1850, "I": 1980}
OTHER = 1800
AREA = 4.0 * math.pi / (POINTS * 1e6)       # a weighted count (count x E^2, thousandths^2) -> A^2


def directions():
    """(128, 3) int64: U[k] = rint(2^20 (r cos k g, r sin k g, z)), z = 1 - (2k + 1) / 128, r = sqrt(1 - z^2), g = pi (3 - sqrt 5)."""
    k = np.arange(POINTS, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / POINTS
    r = np.sqrt(1.0 - z * z)
    g = math.pi * (3.0 - math.sqrt(5.0))
    return np.rint(2.0 ** 20 * np.stack([r * np.cos(k * g), r * np.sin(k * g), z], axis=1)).astype(np.int64)


U = directions()


def offsets(E):
    """The 128 points of an atom of expanded radius E about its centre: (E U + 2^19) >> 20, arithmetic, per component."""
    return (int(E) * U + (1 << 19)) >> 20


def element(record):
    """Columns 77-78 trimmed and upper-cased; a short record or a blank field: the first alphabetic character of 13-16."""
    e = record[76:78].strip().upper() if len(record) >= 78 else ""
    if not e:
        e = next((ch for ch in record[12:16] if ch.isalpha()), "").upper()
    return e


def radius(record):
    """Thousandths; 0 for a record that takes no part (hydrogen, deuterium, a membrane bead)."""
    e = element(record)
    if e in ("H", "D") or record[17:20].strip() == "MMB":
        return 0
    return RADII.get(e, OTHER)


def records(path):
    return [line.rstrip("\r\n") for line in open(path) if line.startswith(("ATOM  ", "HETATM"))]


def file_radii(path):
    return np.array([radius(r) for r in records(path)], dtype=np.int64)


def probe_thousandths(probe):
    assert 0.0 <= probe <= 2.0
    return int(round(1000.0 * probe))


def _pairs(c, bc, reach):
    """Every (i, j) with |c_i - bc_j| <= reach on all three axes, and more: a cell list in numpy.  Only a speed-up."""
    lo = np.minimum(c.min(axis=0), bc.min(axis=0))
    ci, cj = (c - lo) // reach + 1, (bc - lo) // reach + 1
    dims = np.maximum(ci.max(axis=0), cj.max(axis=0)) + 2
    def key(cells):
        return (cells[:, 0] * dims[1] + cells[:, 1]) * dims[2] + cells[:, 2]
    order = np.argsort(key(cj), kind="stable")
    keys = key(cj)[order]
    ii, jj = [], []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                k = key(ci + np.array([dx, dy, dz]))
                left, right = np.searchsorted(keys, k, "left"), np.searchsorted(keys, k, "right")
                n = right - left
                total = int(n.sum())
                if total == 0:
                    continue
                ii.append(np.repeat(np.arange(len(c)), n))
                jj.append(order[np.repeat(left, n) + np.arange(total) - np.repeat(np.cumsum(n) - n, n)])
    if not ii:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(ii), np.concatenate(jj)


def _buried_by(c, E, bc, bE, same, chunk=20000):
    """bool (atoms, 128): point k of atom a of (c, E) lies strictly inside the expanded sphere of some atom of the
    buriers (bc, bE).  same: the buriers ARE the atoms, and an atom never buries itself."""
    out = np.zeros((len(c), POINTS), dtype=bool)
    if len(bc) == 0 or len(c) == 0:
        return out
    pad = 4                                        # a point is at most E_a + 1 from its centre
    i, j = _pairs(c, bc, int(E.max() + bE.max()) + pad)
    d = bc[j] - c[i]
    keep = (d * d).sum(axis=1) < (E[i] + bE[j] + pad) ** 2            # only a speed-up: the test below is the rule
    if same:
        keep &= i != j
    i, j = i[keep], j[keep]
    by_atom = np.argsort(i, kind="stable")
    i, j = i[by_atom], j[by_atom]
    off = (E[:, None, None] * U[None, :, :] + (1 << 19)) >> 20         # (atoms, 128, 3)
    for a in range(0, len(i), chunk):
        ia, ja = i[a:a + chunk], j[a:a + chunk]
        diff = c[ia][:, None, :] + off[ia] - bc[ja][:, None, :]
        hit = (diff * diff).sum(axis=2) < (bE[ja] * bE[ja])[:, None]
        starts = np.flatnonzero(np.r_[True, ia[1:] != ia[:-1]])
        out[ia[starts]] |= np.logical_or.reduceat(hit, starts, axis=0)
    return out


def counts(t, radii, n_rec, probe=1.4):
    """t: (atoms, 3) int64 thousandths of a posed complex, receptor first; radii: thousandths, 0 = takes no part.
    -> (free (atoms,), bound (atoms,), [4 sums as Python ints])."""
    p = probe_thousandths(probe)
    t = np.asarray(t, dtype=np.int64)
    radii = np.asarray(radii, dtype=np.int64)
    part = np.flatnonzero(radii > 0)
    E = radii[part] + p
    c = t[part]
    side = (part >= n_rec).astype(int)
    free = np.zeros(len(radii), dtype=np.int64)
    bound = np.zeros(len(radii), dtype=np.int64)
    sums = []
    for s in (0, 1):
        mine, theirs = np.flatnonzero(side == s), np.flatnonzero(side != s)
        own = _buried_by(c[mine], E[mine], c[mine], E[mine], True)
        other = _buried_by(c[mine], E[mine], c[theirs], E[theirs], False)
        free[part[mine]] = POINTS - own.sum(axis=1)
        bound[part[mine]] = POINTS - (own | other).sum(axis=1)
        E2 = [int(e) * int(e) for e in E[mine]]
        sums.append(sum(int(f) * e2 for f, e2 in zip(free[part[mine]], E2)))
        sums.append(sum(int(b) * e2 for b, e2 in zip(bound[part[mine]], E2)))
    return free, bound, sums


def area(weighted):
    """Weighted counts (count x E^2; a sum of them) -> A^2."""
    return np.asarray(weighted, dtype=np.float64) * AREA


def buried_area(sums):
    s = [int(v) for v in sums]
    return (s[0] - s[1] + s[2] - s[3]) * AREA


class SasaRestated(ContactsRestated):
    def __init__(self, rec_pdb, lig_pdb, rec_modes=None, lig_modes=None):
        ContactsRestated.__init__(self, rec_pdb, lig_pdb, rec_modes, lig_modes)
        self.radii = np.concatenate([file_radii(rec_pdb), file_radii(lig_pdb)])
        self.n_rec = len(self.rec)

    def of_xyz(self, xyz, probe=1.4):
        return counts(thousandths(xyz), self.radii, self.n_rec, probe)

    def sasa(self, row, probe=1.4):
        """One pose -> (free (atoms,), bound (atoms,), [4 sums])."""
        return self.of_xyz(self.pose(row), probe)

    def batch(self, poses, probe=1.4):
        """-> (sums (n, 4) uint64, free (n, atoms) uint8, bound (n, atoms) uint8)."""
        got = [self.sasa(p, probe) for p in poses]
        n_atoms = len(self.radii)
        return (np.array([g[2] for g in got], dtype=np.uint64).reshape(len(got), 4),
                np.array([g[0] for g in got], dtype=np.uint8).reshape(len(got), n_atoms),
                np.array([g[1] for g in got], dtype=np.uint8).reshape(len(got), n_atoms))


def sasa_case(name):
    """A golden case of tests/conftest.py's CASES as a SasaRestated (modes when the case uses them)."""
    from conftest import case_paths
    c, d, rec, lig = case_paths(name)
    if c["use_anm"]:
        return SasaRestated(rec, lig, np.load(os.path.join(d, "rec_nm.npy")), np.load(os.path.join(d, "lig_nm.npy")))
    return SasaRestated(rec, lig)


def czy_sasa():
    from test_analysis_cpu import CZY
    return SasaRestated(os.path.join(CZY, "lightdock_1czy_protein.pdb"), os.path.join(CZY, "lightdock_1czy_peptide.pdb"),
                        np.load(os.path.join(CZY, "lightdock_rec.nm.npy")), np.load(os.path.join(CZY, "lightdock_lig.nm.npy")))


def residue_areas(free, bound, radii, res_of, probe=1.4):
    """Per-residue (free, bound) weighted counts of one side: sum over its atoms of count x E^2."""
    p = probe_thousandths(probe)
    E2 = np.where(radii > 0, (radii + p) ** 2, 0).astype(np.int64)
    n = int(res_of.max()) + 1 if len(res_of) else 0
    out = np.zeros((2, n), dtype=np.int64)
    np.add.at(out[0], res_of, np.asarray(free, dtype=np.int64) * E2)
    np.add.at(out[1], res_of, np.asarray(bound, dtype=np.int64) * E2)
    return out[0], out[1]
