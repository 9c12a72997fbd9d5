"""Clustering by common contacts (include/lightdock_hip.h, "Clustering by common contacts") restated in
int64 numpy: the checker of tests/test_fcc_cpu.py, tests/test_gpu_fcc.py.  Pair sets come from the posing, the thousandths
and the integer atom test of tests/test_contacts_cpu.py; everything after them is integer arithmetic on sets."""
import functools
import os

import numpy as np

from test_analysis_cpu import CZY, tool_module
from test_contacts_cpu import GOLDEN, atom_contacts, case_restated, czy_contacts_restated, thousandths


def threshold_thousandths(threshold):
    T = int(np.rint(threshold * 1000.0))
    assert 1 <= T <= 1000
    return T


# ---- pair sets ----------------------------------------------------------------------------------------------------

def pair_set(rs, row, cutoff=5.0):
    """The ascending keys r * n_lig_res + l of the residue pairs of one pose with an atom pair within the cutoff."""
    n_rec, n_lig_res = len(rs.rec), len(rs.lig_ids)
    t = thousandths(rs.pose(row))
    rec, lig = t[:n_rec], t[n_rec:]
    C = int(round(cutoff * 1000.0))
    # atoms farther than C from the other molecule's box on some axis touch nothing: only a speed-up
    ra = np.flatnonzero(((rec >= lig.min(axis=0) - C) & (rec <= lig.max(axis=0) + C)).all(axis=1))
    la = np.flatnonzero(((lig >= rec.min(axis=0) - C) & (lig <= rec.max(axis=0) + C)).all(axis=1))
    a, b = np.nonzero(atom_contacts(rec[ra], lig[la], cutoff))
    keys = rs.rec_of[ra[a]].astype(np.int64) * n_lig_res + rs.lig_of[la[b]]
    assert len(rs.rec_ids) * n_lig_res < 2 ** 32
    return np.unique(keys)


def to_csr(sets):
    offsets = np.zeros(len(sets) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(s) for s in sets])
    keys = np.concatenate([np.asarray(s, dtype=np.int64) for s in sets]) if len(sets) else np.zeros(0, dtype=np.int64)
    return offsets, keys.astype(np.int64)


def from_csr(offsets, keys):
    return [np.asarray(keys[offsets[i]:offsets[i + 1]], dtype=np.int64) for i in range(len(offsets) - 1)]


def pair_sets(rs, poses, cutoff=5.0):
    """-> (offsets (n + 1,), keys) int64."""
    return to_csr([pair_set(rs, p, cutoff) for p in poses])


def projection(offsets, keys, n_rec_res, n_lig_res):
    """-> (bool (n, receptor residues), bool (n, ligand residues)): the residues the sets' pairs name."""
    n = len(offsets) - 1
    rec, lig = np.zeros((n, n_rec_res), dtype=bool), np.zeros((n, n_lig_res), dtype=bool)
    for i, s in enumerate(from_csr(offsets, keys)):
        rec[i, s // n_lig_res] = True
        lig[i, s % n_lig_res] = True
    return rec, lig


# ---- common contacts, neighbours, clusters, consensus ---------------------------------------------------------------

def membership(offsets, keys):
    """int64 (n, U): 1 where set i holds the u-th distinct key."""
    n = len(offsets) - 1
    union, col = np.unique(np.asarray(keys, dtype=np.int64), return_inverse=True)
    M = np.zeros((n, max(1, len(union))), dtype=np.int64)
    M[np.repeat(np.arange(n), np.diff(offsets)), col] = 1
    return M


def common(offsets, keys):
    """int64 (n, n): c_ij, the diagonal s_i."""
    M = membership(offsets, keys)
    return M @ M.T


def neighbours(c, sizes, T):
    larger = np.maximum(sizes[:, None], sizes[None, :])
    nb = (sizes[:, None] > 0) & (sizes[None, :] > 0) & (1000 * c >= T * larger)
    np.fill_diagonal(nb, False)
    return nb


def consensus(offsets, keys):
    """int64 (n,): the sum over a set's keys of the number of sets that hold the key."""
    M = membership(offsets, keys)
    return M @ M.sum(axis=0)


def cluster(offsets, keys, scoring, threshold=0.6, min_size=1):
    """The greedy rounds, one at a time -> dict of cluster_of, centres (-1 after the last), n_clusters, set_sizes, consensus."""
    offsets, keys = np.asarray(offsets, dtype=np.int64), np.asarray(keys, dtype=np.int64)
    n = len(offsets) - 1
    assert min_size >= 1
    sizes = np.diff(offsets)
    nb = neighbours(common(offsets, keys), sizes, threshold_thousandths(threshold))
    assert np.array_equal(nb, nb.T)
    scoring = np.asarray(scoring, dtype=np.float64)
    alive = np.ones(n, dtype=bool)
    cluster_of, centres = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    k = 0
    while alive.any():
        d = 1 + (nb & alive[None, :]).sum(axis=1)
        idx = np.flatnonzero(alive)
        centre = min(idx, key=lambda i: (-d[i], -scoring[i], i))
        if d[centre] < min_size:
            break
        members = alive & nb[centre]
        members[centre] = True
        cluster_of[members] = k
        centres[k] = centre
        alive &= ~members
        k += 1
    return {"cluster_of": cluster_of, "centres": centres, "n_clusters": k, "set_sizes": sizes, "consensus": consensus(offsets, keys)}


def consensus_fraction(cons, sizes):
    n = len(sizes)
    return np.array([c / float(s * n) if s else 0.0 for c, s in zip(cons, sizes)])


# ---- the committed runs ---------------------------------------------------------------------------------------------

def final_glowworms(case, swarms):
    """Every glowworm of the final step of the swarms, as run_dir.all_glowworms orders them: (poses, scoring, entries)."""
    base = CZY if case == "1czy" else os.path.join(GOLDEN, case)
    entries = tool_module("run_dir").all_glowworms(list(swarms), 100, base=base)
    return np.array([e[2] for e in entries]), np.array([e[3]["scoring"] for e in entries], dtype=np.float64), entries


@functools.lru_cache(maxsize=None)
def run_sets(case, n_swarms):
    """(poses, scoring, entries, offsets, keys, restatement) of the first n_swarms swarms of a committed run at 5 A."""
    rs = czy_contacts_restated() if case == "1czy" else case_restated(case)
    poses, scoring, entries = final_glowworms(case, range(n_swarms))
    offsets, keys = pair_sets(rs, poses[:, :7 + len(rs.rec_modes) + len(rs.lig_modes)])
    return poses, scoring, entries, offsets, keys, rs


@functools.lru_cache(maxsize=None)
def run_clusters(case, n_swarms, threshold=0.6, min_size=1):
    """cluster() on run_sets(case, n_swarms), computed once for the tests that share it."""
    _, scoring, _, offsets, keys, _ = run_sets(case, n_swarms)
    return cluster(offsets, keys, scoring, threshold, min_size)
