"""The density-fit rule of include/lightdock_hip.h ("Density fit") restated in numpy and Python integers,
from the text: the checker of tests/test_emfit_cpu.py and tests/test_gpu_emfit.py.  The simulated voxels are int64 on the
thousandths "%8.3f" prints, the table comes from math.exp, the sums are Python integers, the scores math.sqrt on
correctly rounded float(int).  Posing, rounding and classes are saxs_reference's.  Also what the tool's MRC reader must
return for a header written with struct."""
import math
import os
import struct

import numpy as np

from saxs_reference import NO_PART, SaxsRestated, Z

MAX_TABLE = 4096
VOXEL_LIMIT, SUM_LIMIT = 2 ** 24, 2 ** 40


def kernel_plan(sigma):
    """sigma (thousandths) -> (two, shift, length)."""
    two = 2 * sigma * sigma
    L = math.floor(two * math.log(510.0)) + 1
    s = 0
    while ((L - 1) >> s) + 1 > MAX_TABLE:
        s += 1
    return two, s, ((L - 1) >> s) + 1


def kernel_values(sigma):
    """The unrounded 255 exp(.) of every entry."""
    two, s, T = kernel_plan(sigma)
    return np.array([255.0 * math.exp(-((float(t) + 0.5) * float(1 << s)) / float(two)) for t in range(T)])


def kernel_table(sigma):
    """-> (K (T,) int64, shift)."""
    return np.rint(kernel_values(sigma)).astype(np.int64), kernel_plan(sigma)[1]


def kernel_decided(sigma, eps=1e-9):
    """bool (T,): entries whose value is not within eps of a half-integer, so that libm's last bit cannot move them."""
    v = kernel_values(sigma)
    return np.abs((v - np.floor(v)) - 0.5) > eps


def quantise(rho, threshold=0.0):
    """rho (any shape) float32 -> (E int64, scale), or ValueError."""
    rho = np.asarray(rho, dtype=np.float32).astype(np.float64)
    if not np.isfinite(rho).all():
        raise ValueError("a value is not finite")
    kept = np.where((rho >= threshold) & (rho > 0.0), rho, 0.0)
    top = float(kept.max()) if kept.size else 0.0
    if not top > 0.0:
        raise ValueError("no positive value")
    scale = 32767.0 / top
    return np.rint(kept * scale).astype(np.int64), scale


def centres(n, origin, step):
    """The voxel centres of the three axes, x first, int64."""
    return [origin[k] + np.arange(n[k], dtype=np.int64) * step[k] for k in range(3)]


def simulate(t, weights, n, origin, step, table, shift):
    """t (atoms, 3) int64 thousandths, weights (atoms,) -> (nz, ny, nx) int64: every atom adds w K[d2 >> shift] to every
    voxel of the grid with d2 < len(K) << shift."""
    X, Y, Zc = centres(n, origin, step)
    limit = len(table) << shift
    grid = np.zeros((n[2], n[1], n[0]), dtype=np.int64)
    for (x, y, z), w in zip(np.asarray(t, dtype=np.int64).tolist(), list(weights)):
        dx, dy, dz = (X - x) ** 2, (Y - y) ** 2, (Zc - z) ** 2
        ix, iy, iz = np.flatnonzero(dx < limit), np.flatnonzero(dy < limit), np.flatnonzero(dz < limit)
        if not (len(ix) and len(iy) and len(iz)):
            continue
        d2 = dz[iz][:, None, None] + dy[iy][None, :, None] + dx[ix][None, None, :]
        add = np.where(d2 < limit, table[np.minimum(d2 >> shift, len(table) - 1)], 0) * int(w)
        grid[iz[0]:iz[-1] + 1, iy[0]:iy[-1] + 1, ix[0]:ix[-1] + 1] += add
    return grid


def outside_count(t, n, origin, step):
    t = np.asarray(t, dtype=np.int64).reshape(-1, 3)
    out = np.zeros(len(t), dtype=bool)
    for k in range(3):
        first, last = origin[k], origin[k] + (n[k] - 1) * step[k]
        out |= (2 * (t[:, k] - first) < -step[k]) | (2 * (t[:, k] - last) >= step[k])
    return int(out.sum())


def sums_of(grid, E):
    """The four sums as Python integers; ValueError past the two limits."""
    g, e = [int(v) for v in np.asarray(grid).ravel()], [int(v) for v in np.asarray(E).ravel()]
    s, ss, se, inside = sum(g), sum(v * v for v in g), sum(v * w for v, w in zip(g, e)), sum(v for v, w in zip(g, e) if w > 0)
    if (g and max(g) >= VOXEL_LIMIT) or s >= SUM_LIMIT:
        raise ValueError("overflow")
    return {"s": s, "ss": ss, "se": se, "inside_sum": inside}


def scores(N, S_e, S_ee, s, ss, se, inside_sum):
    """-> (cc, ccm, inside) with Python integers and math.sqrt."""
    cc = 0.0 if ss == 0 else float(se) / (math.sqrt(float(ss)) * math.sqrt(float(S_ee)))
    A, B, Cc = N * se - s * S_e, N * ss - s * s, N * S_ee - S_e * S_e
    ccm = 0.0 if B == 0 or Cc == 0 else float(A) / (math.sqrt(float(B)) * math.sqrt(float(Cc)))
    return cc, ccm, (0.0 if s == 0 else float(inside_sum) / float(s))


class EmfitRestated(SaxsRestated):
    """A complex and a map: rho (nz, ny, nx), origin and step (x, y, z) in thousandths."""

    def __init__(self, rec_pdb, lig_pdb, rec_modes=None, lig_modes=None):
        SaxsRestated.__init__(self, rec_pdb, lig_pdb, rec_modes, lig_modes)
        self.part = np.flatnonzero(self.classes != NO_PART)
        self.weights = np.array([Z[c] for c in self.classes[self.part]], dtype=np.int64)

    def grid(self, row, shape, origin, step, sigma):
        table, shift = kernel_table(sigma)
        n = (shape[2], shape[1], shape[0])
        return simulate(self.thousandths(row)[self.part], self.weights, n, origin, step, table, shift)

    def fit(self, row, E, origin, step, sigma):
        """One pose -> (the dict of density_fit's words, the grid)."""
        E = np.asarray(E)
        grid = self.grid(row, E.shape, origin, step, sigma)
        out = sums_of(grid, E)
        out["outside"] = outside_count(self.thousandths(row)[self.part], (E.shape[2], E.shape[1], E.shape[0]), origin, step)
        return out, grid


def same_words(got, want_rows):
    """density_fit's dict against a list of fit() dicts."""
    return all([int(v) for v in got[k]] == [w[k] for w in want_rows] for k in ("s", "ss", "se", "inside_sum", "outside"))


def czy_emfit():
    from test_analysis_cpu import CZY
    return EmfitRestated(os.path.join(CZY, "lightdock_1czy_protein.pdb"), os.path.join(CZY, "lightdock_1czy_peptide.pdb"),
                         np.load(os.path.join(CZY, "lightdock_rec.nm.npy")), np.load(os.path.join(CZY, "lightdock_lig.nm.npy")))


# ---- MRC files, written with struct ---------------------------------------------------------------------------------

MRC_DTYPES = {0: "i1", 1: "i2", 2: "f4", 6: "u2"}


def mrc_bytes(data, mode, order="<", axes=(1, 2, 3), nstart=(0, 0, 0), m=None, cella=None, angles=(90.0, 90.0, 90.0), origin=(0.0, 0.0, 0.0),
              extended=b"", stamp=None):
    """data (sections, rows, columns) in FILE order -> the bytes of an MRC2014 file.  m, cella: per space axis x, y, z."""
    ns, nr, nc = data.shape
    head = bytearray(1024)
    struct.pack_into(order + "10i", head, 0, nc, nr, ns, mode, nstart[0], nstart[1], nstart[2], m[0], m[1], m[2])
    struct.pack_into(order + "6f", head, 40, cella[0], cella[1], cella[2], *angles)
    struct.pack_into(order + "3i", head, 64, *axes)
    struct.pack_into(order + "2i", head, 88, 1, len(extended))
    struct.pack_into(order + "3f", head, 196, *origin)
    head[208:212] = b"MAP "
    head[212:216] = stamp if stamp is not None else (bytes([0x44, 0x44, 0, 0]) if order == "<" else bytes([0x11, 0x11, 0, 0]))
    body = np.ascontiguousarray(data).astype(np.dtype(order + MRC_DTYPES.get(mode, "f4"))).tobytes()
    return bytes(head) + extended + body
