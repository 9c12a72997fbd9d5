"""TEST INFRASTRUCTURE: the rule of include/lightdock_hip.h, "Normal modes", restated in numpy with numpy.linalg.eigh as the
eigensolver, and the bounds the GPU solver is held to.  Nothing here calls the library; tests/test_anm_cpu.py checks this
restatement against the mode files under tests/golden, which ProDy wrote.

Bounds (n = 3 m, lambda from eigh): an eigenvalue within 64 n 2^-53 lambda_max; a node eigenvector within
64 n 2^-53 lambda_max / gap_k after sign alignment, gap_k the smaller distance to a neighbouring eigenvalue -- the
first-order perturbation bound of a symmetric eigenproblem solved backward-stably, 64 covering both solvers' rounding.
"""
import numpy as np

RIGID = 6
CUTOFF = 15.0


def read_pdb(path):
    """(names, residue keys, xyz) of the ATOM / HETATM records in file order; a residue key is columns 18-20 and 22-27."""
    names, keys, xyz = [], [], []
    with open(path) as f:
        for line in f:
            if line.startswith("ATOM  ") or line.startswith("HETATM"):
                names.append(line[12:16].strip())
                keys.append((line[17:20], line[21:27]))
                xyz.append([float(line[30:38]), float(line[38:46]), float(line[46:54])])
    return names, keys, np.array(xyz)


def residues(keys):
    """res_of_atom: maximal runs of consecutive records with one key."""
    res = np.zeros(len(keys), dtype=np.int64)
    for a in range(1, len(keys)):
        res[a] = res[a - 1] + (keys[a] != keys[a - 1])
    return res


def residue_id(key):
    resname, rest = key
    return "%s.%s.%d%s" % (rest[0].strip(), resname.strip(), int(rest[1:5]), rest[5].strip())


def node_atoms(names, res):
    """The node atom of every residue: its first CA, else its first C4'; ValueError naming the residue index otherwise."""
    out = []
    for r in range(int(res[-1]) + 1):
        atoms = np.nonzero(res == r)[0]
        ca = [a for a in atoms if names[a] == "CA"]
        c4 = [a for a in atoms if names[a] == "C4'"]
        if not ca and not c4:
            raise ValueError("residue %d has no node atom" % r)
        out.append(ca[0] if ca else c4[0])
    return np.array(out)


def hessian(xyz, cutoff=CUTOFF):
    xyz = np.asarray(xyz, dtype=np.float64)
    m = xyz.shape[0]
    H = np.zeros((3 * m, 3 * m))
    for i in range(m):
        d = xyz - xyz[i]
        d2 = np.einsum("ij,ij->i", d, d)
        diag = np.zeros((3, 3))
        for j in np.nonzero((d2 > 0.0) & (d2 <= cutoff * cutoff))[0]:
            if j == i:
                continue
            block = np.outer(d[j], d[j]) * (-1.0 / d2[j])
            H[3 * i:3 * i + 3, 3 * j:3 * j + 3] = block
            diag += block
        H[3 * i:3 * i + 3, 3 * i:3 * i + 3] = -diag
    return H


def eigen(xyz, cutoff=CUTOFF):
    """All eigenpairs ascending: (values (n,), vectors as columns)."""
    return np.linalg.eigh(hessian(xyz, cutoff))


def fix_sign(v):
    """The component of largest magnitude (lowest index on a tie) positive."""
    at = int(np.argmax(np.abs(v)))
    return -v if v[at] < 0 else v


def node_modes(xyz, k, cutoff=CUTOFF):
    """(k eigenvalues, modes (k, m, 3) of unit norm with the sign rule, all eigenvalues)."""
    w, v = eigen(xyz, cutoff)
    m = len(xyz)
    modes = np.array([fix_sign(v[:, RIGID + r] / np.linalg.norm(v[:, RIGID + r])).reshape(m, 3) for r in range(k)])
    return w[RIGID:RIGID + k], modes, w


def atom_modes(path, k, cutoff=CUTOFF, rmsd=0.0):
    """(eigenvalues, modes (k, atoms, 3)) of a PDB file by the whole rule."""
    names, keys, xyz = read_pdb(path)
    res = residues(keys)
    nodes = node_atoms(names, res)
    lam, modes, _ = node_modes(xyz[nodes], k, cutoff)
    out = modes[:, res, :]
    out = out / np.sqrt((out ** 2).sum(axis=(1, 2)))[:, None, None]
    if rmsd > 0.0:
        scale = rmsd * np.sqrt(len(res)) / np.sqrt((1.0 / lam).sum()) / np.sqrt(lam)
        out = out * scale[:, None, None]
    return lam, out


def bounds(w, k):
    """(eigenvalue bound, eigenvector bound of each of the k modes) from ALL eigenvalues w, ascending."""
    n = len(w)
    base = 64.0 * n * 2.0 ** -53 * w[-1]
    gaps = []
    for r in range(RIGID, RIGID + k):
        g = w[r] - w[r - 1]
        if r + 1 < n:
            g = min(g, w[r + 1] - w[r])
        gaps.append(g)
    return base, base / np.array(gaps)


def align(got, want):
    """`got` with the sign that brings it nearest to `want`."""
    return got if np.abs(got - want).max() <= np.abs(got + want).max() else -got
