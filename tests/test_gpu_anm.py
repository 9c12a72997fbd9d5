"""Normal modes on the GPU (ld_anm_modes / ld_anm_modes_xyz) against the mode files under tests/golden and
against tests/anm_reference.py, the rule in numpy with numpy.linalg.eigh.

Bounds, derived (anm_reference.bounds; n = 3 m, lambda from eigh): an eigenvalue within 64 n 2^-53 lambda_max; node
eigenvector k within 64 n 2^-53 lambda_max / gap_k after sign alignment, gap_k the smaller distance to a neighbouring
eigenvalue.  An atom's component is its node's divided by a norm >= 1, so the same bound holds for the atom modes; the
goldens get 1e-13 on top, what the numpy restatement itself differs from them (tests/test_anm_cpu.py).  Wanted eigenvalues
closer than 1e-8 relative are compared as one projector, the gap being the cluster's distance to the rest."""
import ctypes as C
import functools
import json
import os
import shutil

import numpy as np
import pytest

import anm_reference as ar
from conftest import GOLDEN
from test_anm_cpu import MOLECULES, golden_modes

pytestmark = pytest.mark.gpu

K = 10


@functools.lru_cache(maxsize=None)
def reference_of(name):
    """(all eigenvalues, eigenvalue bound, eigenvector bounds of the ten modes) of a golden molecule's network."""
    names, keys, xyz = ar.read_pdb(os.path.join(GOLDEN, MOLECULES[name][0]))
    w = np.linalg.eigvalsh(ar.hessian(xyz[ar.node_atoms(names, ar.residues(keys))]))
    return (w,) + ar.bounds(w, K)


@pytest.fixture(scope="module")
def anm(pkg):
    pkg.init(0)
    return pkg


@pytest.mark.parametrize("name", ["2uuy_rec", "2uuy_lig", "1azp_rec", "1azp_dna", "ab_icode_rec"])
def test_golden_unit_modes(anm, name):
    w, eig_bound, vec_bound = reference_of(name)
    eig, modes = anm.anm_modes(os.path.join(GOLDEN, MOLECULES[name][0]), K)
    gold = golden_modes(name)
    err = np.array([np.abs(ar.align(modes[r], gold[r]) - gold[r]).max() for r in range(K)])
    print(name, "eigenvalue error / bound %.3g" % (np.abs(eig - w[6:6 + K]).max() / eig_bound),
          "mode error / bound", np.array2string(err / (vec_bound + 1e-13), precision=3), "%.1f ms" % anm.anm_last_kernel_ms())
    assert np.all(np.abs(eig - w[6:6 + K]) <= eig_bound)
    assert np.all(err <= vec_bound + 1e-13)
    assert np.allclose((modes ** 2).sum(axis=(1, 2)), 1.0, rtol=0, atol=1e-13)


@pytest.mark.parametrize("name", ["1czy_rec", "1czy_lig"])
def test_golden_scaled_modes(anm, name):
    """The 1czy files hold c / sqrt(lambda_k) times the unit mode: the directions match within the bound; with rmsd = 0.5
    golden / ours is one factor for all ten modes (the library's amplitude is the expectation of the sample ProDy drew)."""
    w, eig_bound, vec_bound = reference_of(name)
    path = os.path.join(GOLDEN, MOLECULES[name][0])
    eig, modes = anm.anm_modes(path, K)
    gold = golden_modes(name)
    unit = gold / np.sqrt((gold ** 2).sum(axis=(1, 2)))[:, None, None]
    err = np.array([np.abs(ar.align(modes[r], unit[r]) - unit[r]).max() for r in range(K)])
    print(name, "mode error / bound", np.array2string(err / (vec_bound + 1e-13), precision=3))
    assert np.all(np.abs(eig - w[6:6 + K]) <= eig_bound)
    assert np.all(err <= vec_bound + 1e-13)
    eig2, scaled = anm.anm_modes(path, K, rmsd=0.5)
    assert np.array_equal(eig, eig2)
    factor = np.array([abs((gold[r] * scaled[r]).sum() / (scaled[r] ** 2).sum()) for r in range(K)])
    print(name, "golden / ours", factor)
    assert np.ptp(factor) <= 1e-9 * factor[0]
    assert 0.9 <= factor[0] <= 1.2


def helix(m, seed=0):
    """m nodes that hold together: a jittered helix, about 3.8 A between neighbours."""
    rng = np.random.default_rng(seed)
    i = np.arange(m)
    return np.stack([5.0 * np.cos(1.7 * i), 5.0 * np.sin(1.7 * i), 1.5 * i], axis=1) + rng.uniform(-0.5, 0.5, (m, 3))


def peptide_nodes():
    names, keys, xyz = ar.read_pdb(os.path.join(GOLDEN, MOLECULES["1czy_lig"][0]))
    return xyz[ar.node_atoms(names, ar.residues(keys))]


SHAPES = {
    "tetrahedron_n12": (lambda: np.array([[0, 0, 0], [3.8, 0.2, 0], [1.1, 3.5, 0.4], [1.6, 1.2, 3.3]], dtype=np.float64), 6),
    "five_n15": (lambda: helix(5, 1), 9),
    "peptide_n21": (peptide_nodes, 10),
    "wave_n66": (lambda: helix(22, 2), 10),
    "workgroup_n258": (lambda: helix(86, 3), 10),
}


def clusters(lam):
    """Runs of wanted eigenvalues closer than 1e-8 relative, as (first, last + 1)."""
    runs, start = [], 0
    for r in range(1, len(lam) + 1):
        if r == len(lam) or lam[r] - lam[r - 1] > 1e-8 * lam[r]:
            runs.append((start, r))
            start = r
    return runs


def compare_with_reference(anm, xyz, k, label):
    lam, want, w = ar.node_modes(xyz, k)
    n = len(w)
    base = 64.0 * n * 2.0 ** -53 * w[-1]
    eig, got = anm.anm_modes_xyz(xyz, k)
    assert np.all(np.abs(eig - lam) <= base), (label, np.abs(eig - lam).max() / base)
    assert np.all(np.diff(eig) >= 0)
    worst = 0.0
    for a, b in clusters(lam):
        gap = lam[a] - w[6 + a - 1]
        if 6 + b < n:
            gap = min(gap, w[6 + b] - lam[b - 1])
        if b - a == 1:
            err = np.abs(ar.align(got[a], want[a]) - want[a]).max()
        else:
            G, W = got[a:b].reshape(b - a, -1), want[a:b].reshape(b - a, -1)
            err = np.abs(G.T @ G - W.T @ W).max()
        worst = max(worst, err * gap / base)
        assert err <= base / gap, (label, a, b, err, base / gap)
    print(label, "n", n, "eigenvalue error / bound %.3g" % (np.abs(eig - lam).max() / base), "worst mode error / bound %.3g" % worst)
    flat = got.reshape(k, -1)
    assert np.allclose(flat @ flat.T, np.eye(k), rtol=0, atol=1e-12)
    # the sign rule; components that tie to the last bits (a lattice's symmetric modes) may be of either sign
    assert np.all(flat.max(axis=1) >= np.abs(flat).max(axis=1) * (1.0 - 1e-12))
    return eig, got


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_smallest_shapes_against_numpy(anm, shape):
    make, k = SHAPES[shape]
    compare_with_reference(anm, make(), k, shape)


def test_cubic_lattice_with_degenerate_modes(anm):
    g = np.arange(3) * 6.0
    xyz = np.array([[x, y, z] for x in g for y in g for z in g])
    w = np.linalg.eigvalsh(ar.hessian(xyz))
    # the cut falls between clusters: the largest k <= 12 whose last mode is well apart from the next
    k = max(k for k in range(4, 13) if w[6 + k] - w[6 + k - 1] > 1e-3)
    lam = w[6:6 + k]
    assert any(b - a > 1 for a, b in clusters(lam))   # the lattice does have exactly degenerate modes among them
    compare_with_reference(anm, xyz, k, "lattice k=%d" % k)


def raw_call(anm, xyz, m, k, cutoff=15.0):
    """ld_anm_modes_xyz on sentinel outputs -> (status, outputs untouched)."""
    lib = anm.load_library()
    xyz = np.ascontiguousarray(xyz, dtype=np.float64)
    modes, eig = np.full(max(1, k) * max(1, m) * 3, -7.0), np.full(max(1, k), -7.0)
    rc = lib.ld_anm_modes_xyz(xyz.ctypes.data_as(C.c_void_p), m, k, C.c_double(cutoff), modes.ctypes.data_as(C.c_void_p),
                              eig.ctypes.data_as(C.c_void_p))
    return rc, bool(np.all(modes == -7.0) and np.all(eig == -7.0))


def test_refusals_leave_the_outputs_untouched(anm, tmp_path):
    ten = helix(10, 4)
    apart = np.concatenate([ten, ten + [100.0, 0.0, 0.0]])
    line = np.stack([3.8 * np.arange(5), np.zeros(5), np.zeros(5)], axis=1)
    bad = ten.copy()
    bad[5, 2] = np.nan
    cases = {"3 nodes, 4 modes": (helix(3), 3, 4), "4 nodes, 7 modes": (helix(4), 4, 7), "two clusters": (apart, 20, 10),
             "collinear": (line, 5, 4), "NaN": (bad, 10, 10), "k = 0": (ten, 10, 0), "k = 129": (helix(50), 50, 129),
             "m = 4097": (np.zeros((4097, 3)), 4097, 10)}
    for label, (xyz, m, k) in cases.items():
        rc, untouched = raw_call(anm, xyz, m, k)
        assert rc == -1 and untouched, label
        assert anm.load_library().ld_last_error(), label
    path = tmp_path / "no_node.pdb"
    names, keys, _ = ar.read_pdb(os.path.join(GOLDEN, MOLECULES["1czy_lig"][0]))
    res = ar.residues(keys)
    atoms = [l for l in open(os.path.join(GOLDEN, MOLECULES["1czy_lig"][0])) if l.startswith("ATOM  ") or l.startswith("HETATM")]
    path.write_text("".join(l for a, l in enumerate(atoms) if not (res[a] == 2 and names[a] == "CA")))
    modes = np.full(3 * len(atoms) * 3, -7.0)
    rc = anm.load_library().ld_anm_modes(os.fsencode(str(path)), 3, C.c_double(15.0), C.c_double(0.0), modes.ctypes.data_as(C.c_void_p), None)
    assert rc == -1 and np.all(modes == -7.0)
    assert ar.residue_id(keys[int(np.nonzero(res == 2)[0][0])]) in anm.load_library().ld_last_error().decode()


def test_same_bits_on_every_call(anm):
    a, b = helix(86, 3), peptide_nodes()
    eig_a, modes_a = anm.anm_modes_xyz(a, 10)
    again = anm.anm_modes_xyz(a, 10)
    assert np.array_equal(eig_a, again[0]) and np.array_equal(modes_a, again[1])
    anm.anm_modes_xyz(b, 10)
    after = anm.anm_modes_xyz(a, 10)
    assert np.array_equal(eig_a, after[0]) and np.array_equal(modes_a, after[1])
    path = os.path.join(GOLDEN, MOLECULES["1azp_dna"][0])
    first, second = anm.anm_modes(path, K), anm.anm_modes(path, K)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
    assert anm.anm_last_kernel_ms() > 0.0


def test_the_tool_writes_what_a_run_reads(anm, tmp_path, monkeypatch):
    import lightdock_rust_amd.anm as tool
    import lightdock_rust_amd.launch as launch
    src = os.path.join(GOLDEN, "2uuy")
    for f in ("setup.json", "lightdock_2UUY_rec.pdb", "lightdock_2UUY_lig.pdb"):
        shutil.copy(os.path.join(src, f), tmp_path / f)
    monkeypatch.chdir(tmp_path)
    setup = str(tmp_path / "setup.json")
    assert tool.main([setup]) == 0
    k = json.load(open(setup))["anm_rec"]
    for side, name in (("rec", "2uuy_rec"), ("lig", "2uuy_lig")):
        atoms = MOLECULES[name][2]
        shaped, flat = np.load("lightdock_%s.nm.npy" % side), np.load("%s_nm.npy" % side)
        assert shaped.shape == (k, atoms, 3) and shaped.dtype == np.dtype("<f8")
        assert flat.shape == (k * atoms * 3,) and flat.dtype == np.dtype("<f8") and np.array_equal(flat, shaped.reshape(-1))
        assert np.array_equal(launch.load_nmodes(side, str(tmp_path)), flat)
        gold = golden_modes(name)
        _, _, vec_bound = reference_of(name)
        assert all(np.abs(ar.align(shaped[r], gold[r]) - gold[r]).max() <= vec_bound[r] + 1e-13 for r in range(k))
    before = {f: open(f, "rb").read() for f in os.listdir(".")}
    os.remove("lig_nm.npy")            # one file of four left out: still a refusal, and nothing is written
    del before["lig_nm.npy"]
    assert tool.main([setup]) != 0
    assert {f: open(f, "rb").read() for f in os.listdir(".")} == before
    assert tool.main([setup, "--force"]) == 0 and os.path.exists("lig_nm.npy")
