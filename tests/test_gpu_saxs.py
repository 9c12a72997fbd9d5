"""Small-angle scattering on the MI355X (ld_complex_distance_histogram, ld_saxs_debye, ld_complex_saxs,
lightdock-rust_amd/saxs.py).  Counts are compared word for word with the int64 numpy restatement of
tests/saxs_reference.py; intensities bit for bit with its ordered Debye loop on the library's own tables."""
import ctypes
import hashlib
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import saxs_reference as sx
from test_analysis_cpu import CZY, analyse_module
from test_gpu_contacts import REC, LIG, perturbed_czy
from test_gpu_sasa import atom, pair_of_files

pytestmark = pytest.mark.gpu

FILL = 0xA5
TILE = 256                       # kSaxsTile of kernels/saxs.hpp
Q = np.array([0.0, 0.01, 0.05, 0.1, 0.2, 0.35, 0.5, 1.0])
CO = sx.pair_class(1, 3)
OWN_TABLES_RTOL = 1e-12           # a profile against the restatement on ITS OWN tables (shared with tests/test_gpu_handle_history.py)


def rigid(t):
    t = np.asarray(t, dtype=np.float64).reshape(-1, 3)
    poses = np.zeros((len(t), 7))
    poses[:, :3] = t
    poses[:, 3] = 1.0
    return poses


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def only_pair(row):
    """(class, bin) of the one pair of a (21, bins) row."""
    at = np.argwhere(row)
    assert len(at) == 1 and row[tuple(at[0])] == 1
    return int(at[0][0]), int(at[0][1])


@pytest.fixture(scope="module")
def two_atoms(pkg, tmp_path_factory):
    pkg.init(0)
    rec, lig = pair_of_files(tmp_path_factory.mktemp("co"), atom(1, "C", "GLY", "A", 1, (0, 0, 0), "C"), atom(1, "O", "HOH", "B", 1, (0, 0, 0), "O"))
    return pkg.Complex(rec, lig), sx.SaxsRestated(rec, lig)


@pytest.fixture(scope="module")
def czy(pkg):
    pkg.init(0)
    return pkg.Complex(REC, LIG, np.load(os.path.join(CZY, "lightdock_rec.nm.npy")), 10,
                       np.load(os.path.join(CZY, "lightdock_lig.nm.npy")), 10)


@pytest.fixture(scope="module")
def czy_rs():
    return sx.czy_saxs()


@pytest.fixture(scope="module")
def ranked():
    """Five of the eleven ranked models of the 1czy run and their restated counts at 0.5 A, 400 bins: made once."""
    entries = analyse_module().ranking(range(10), 100, base=CZY)
    poses = np.array([e[2] for e in entries])[[0, 2, 5, 8, 10]]
    return poses, sx.czy_saxs().batch(poses, 500, 400)


# ---- 1. knife edges ---------------------------------------------------------------------------------------------

def test_knife_edges_of_a_bin(pkg, two_atoms):
    cx, rs = two_atoms
    w, bins = 500, 8
    t = [(k * 0.5, 0, 0) for k in range(8)] + [(k * 0.5 - 0.001, 0, 0) for k in range(1, 9)]
    want = list(range(8)) + list(range(8))                 # printed distance k w -> bin k; k w - 1 -> bin k - 1
    t += [(0.3, 0.4, 0), (0.299, 0.4, 0), (0, -3.999, 0), (0, 0, 0.4996), (0, 0, -0.4994), (-1.2, 1.6, 0.001), (1.2, -1.6, 0)]
    want += [1, 0, 7, 1, 0, 4, 4]
    poses = rigid(t)
    got = cx.distance_histogram(poses, w / 1000.0, bins)
    assert got.dtype == np.uint32 and got.shape == (len(t), 21, bins)
    assert [only_pair(r) for r in got] == [(CO, k) for k in want]
    assert np.array_equal(got, rs.batch(poses, w, bins))
    # the last bin is accepted; one bin beyond it is refused and nothing is written
    lib = pkg.load_library()
    for tx, status in ((3.999, 0), (4.0, -1), (4.5, -1)):
        p = rigid([(0.1, 0, 0), (tx, 0, 0), (0.2, 0, 0)])
        buf = np.full((3, 21, bins), 0xA5A5A5A5, dtype=np.uint32)
        assert lib.ld_complex_distance_histogram(cx._h, 3, p.ctypes.data_as(ctypes.c_void_p), 7, w, bins, buf.ctypes.data_as(ctypes.c_void_p)) == status
        assert (buf == 0xA5A5A5A5).all() == (status != 0)
        if status:
            assert "beyond the last bin" in lib.ld_last_error().decode()
            with pytest.raises(pkg.LightdockError):
                cx.distance_histogram(p, w / 1000.0, bins)
    assert only_pair(cx.distance_histogram(rigid([(4.0, 0, 0)]), w / 1000.0, 9)[0]) == (CO, 8)


def test_exactness_at_the_top_of_the_range(pkg, two_atoms):
    """Near 2 x 10^6 thousandths a thousandth off the axis moves d^2 by 1 in 4 x 10^12: f32 cannot see it, the two 64-bit
    compares do."""
    cx, rs = two_atoms
    # 2 000 000^2 is the edge of bin 1000 at w = 2000: (1 999 999, 2000) is 4e12 - 4e6 + 1 + 4e6 = 4e12 + 1 -> bin 1000
    t = [(1999.999, 2.0, 0), (1999.999, 1.999, 0), (2000.0, 0, 0), (1999.999, 0, 0), (1999.999, 0.001, 0), (-2047.999, 0, 0.001),
         (1182.413, -1182.413, 1182.413)]
    poses = rigid(t)
    got = cx.distance_histogram(poses, 2.0, 1024)
    assert [only_pair(r)[1] for r in got] == [1000, 999, 1000, 999, 999, 1023, 1023]
    assert np.array_equal(got, rs.batch(poses, 2000, 1024))
    for far in ((2048.0, 0, 0), (1182.414, -1182.414, 1182.414), (5000.0, 0, 0), (4194.304, 4194.304, 4194.304), (9.0e5, -9.0e5, 9.0e5)):
        with pytest.raises(pkg.LightdockError):
            cx.distance_histogram(rigid([far]), 2.0, 1024)
    # the narrowest bins at their top
    got = cx.distance_histogram(rigid([(102.399, 0.001, 0), (60.0, 80.0, 0), (59.999, 80.0, 0)]), 0.1, 1024)
    assert [only_pair(r)[1] for r in got] == [1023, 1000, 999]


# ---- 2. classes -------------------------------------------------------------------------------------------------

def test_all_six_elements_a_deuterium_a_bead_and_a_zinc(pkg, tmp_path):
    pkg.init(0)
    rec = (atom(1, "H", "GLY", "A", 1, (0, 0, 0), "H") + atom(2, "C", "GLY", "A", 1, (1.1, 0, 0), "C") + atom(3, "N", "GLY", "A", 1, (0, 1.3, 0), "N") +
           atom(4, "O", "GLY", "A", 1, (0, 0, 1.7), "O") + atom(5, "P", "DA", "A", 2, (2.3, 2.3, 0), "P") + atom(6, "SG", "CYS", "A", 3, (0, 2.9, 2.9), "S") +
           atom(7, "ZN", "ZN", "A", 4, (0.5, 0.5, 0.5), "ZN", True) + atom(8, "BJ", "MMB", "A", 5, (0.7, 0.7, 0.7), "C", True))
    lig = (atom(1, "D1", "GLY", "B", 1, (3.1, 0, 0), "D") + atom(2, "CA", "GLY", "B", 1, (0, 3.7, 0), "") + atom(3, "N", "GLY", "B", 1, (0, 0, 4.1), "n") +
           atom(4, "O", "HOH", "B", 2, (4.3, 4.3, 0), " O", True) + atom(5, "P", "DT", "B", 3, (0, 4.7, 4.7), "P") + atom(6, "SD", "MET", "B", 4, (5.3, 0, 5.3), "S") +
           "ATOM      7 1HB  ALA B   5    %8.3f%8.3f%8.3f\n" % (5.9, 5.9, 5.9))
    rec, lig = pair_of_files(tmp_path, rec, lig)
    cx, rs = pkg.Complex(rec, lig), sx.SaxsRestated(rec, lig)
    assert list(cx.saxs_classes(0)) == [0, 1, 2, 3, 4, 5, 255, 255] and list(cx.saxs_classes(1)) == [0, 1, 2, 3, 4, 5, 0]
    assert np.array_equal(np.concatenate([cx.saxs_classes(0), cx.saxs_classes(1)]), rs.classes) and list(rs.n_e) == [3, 2, 2, 2, 2, 2]
    with pytest.raises(pkg.LightdockError):
        cx.saxs_classes(2)
    poses = rigid([(0, 0, 0), (-1.234, 0.777, 2.001)])
    poses[1, 3:7] = [0.5, 0.5, -0.5, 0.5]
    got = cx.distance_histogram(poses, 0.4, 40)
    assert np.array_equal(got, rs.batch(poses, 400, 40))
    assert (got.sum(axis=2) > 0).all() and (got.sum(axis=(1, 2)) == 13 * 12 // 2).all()      # every one of the 21 pair classes is hit
    for name in ("1azp", "1k4c"):
        from test_gpu_contacts import case_complex
        from conftest import case_paths
        _, _, r, l = case_paths(name)
        big = case_complex(pkg, name)
        assert np.array_equal(np.concatenate([big.saxs_classes(0), big.saxs_classes(1)]), np.concatenate([sx.file_classes(r), sx.file_classes(l)]))


# ---- 3. shapes --------------------------------------------------------------------------------------------------

ELEMENTS = ("C", "N", "O", "S", "H", "P")


def random_file(rng, n, chain, first=0):
    xyz = rng.uniform(-20.0, 20.0, (n, 3))
    return "".join(atom(i + 1, ELEMENTS[(first + i) % 6], "UNK", chain, i + 1, xyz[i], ELEMENTS[(first + i) % 6]) for i in range(n))


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
@pytest.mark.parametrize("one", ["receptor", "ligand"])
def test_sizes_around_the_wave_and_the_tile(pkg, tmp_path, n, one):
    """n atoms take part, random in a box of 40 A; a one-atom receptor with the rest in the ligand, or the reverse.  A zinc
    fills the side that would be empty, and takes no part."""
    pkg.init(0)
    rng = np.random.default_rng(1000 + n)
    single = random_file(rng, 1, "A")
    rest = random_file(rng, n - 1, "B", 1) if n > 1 else atom(1, "ZN", "ZN", "B", 1, (3.0, 3.0, 3.0), "ZN", True)
    rec, lig = pair_of_files(tmp_path, *((single, rest) if one == "receptor" else (rest, single)))
    cx, rs = pkg.Complex(rec, lig), sx.SaxsRestated(rec, lig)
    assert rs.n_part == n
    poses = rigid([(0, 0, 0), (3.3, -2.2, 1.1), (-4.0, 0.5, 2.5)])
    poses[1, 3:7] = [0.1, -0.7, 0.3, 0.64]                 # not normalised: the posing divides by the norm
    poses[2, 3:7] = [0.0, 0.0, 1.0, 0.0]
    # 17 KB and 86 KB of LDS, and the two bin counts between which the launch asks for more than the default 64 KB;
    # 40 sqrt(3) + 4.8 A fit all four
    for w, bins in ((500, 200), (100, 1024), (150, 731), (150, 732)):
        got, want = cx.distance_histogram(poses, w / 1000.0, bins), rs.batch(poses, w, bins)
        assert np.array_equal(got, want)
        assert (got.sum(axis=(1, 2), dtype=np.int64) == n * (n - 1) // 2).all()
    I, counts = cx.saxs(poses, Q, 0.5, 200, counts=True)
    assert np.array_equal(counts, rs.batch(poses, 500, 200))
    f, s = pkg.saxs_form_factors(Q), pkg.saxs_sinc(Q, 0.5, 200)
    assert same_bits(I, np.array([rs.profile(c, f, s) for c in counts]))


# ---- 4. 1czy with its modes -------------------------------------------------------------------------------------

def test_1czy_ranked_models(czy, czy_rs, ranked):
    poses, want = ranked
    got = czy.distance_histogram(poses, 0.5, 400)
    assert np.array_equal(got, want)
    n = czy_rs.n_part
    assert n == int((czy_rs.classes != 255).sum()) and (got.sum(axis=(1, 2), dtype=np.int64) == n * (n - 1) // 2).all()
    assert np.array_equal(czy.distance_histogram(poses, 0.5, 1024)[:, :, :400], want)


def test_batches_of_1_7_and_300_give_identical_rows(czy, ranked):
    poses, want = ranked
    filler = perturbed_czy(np.random.default_rng(8), 2).reshape(-1, 27)[:300]
    for i, p in enumerate(poses):
        assert np.array_equal(czy.distance_histogram(p[None, :], 0.5, 400)[0], want[i])
    seven = filler[:7].copy()
    seven[[1, 2, 4, 5, 6]] = poses
    assert np.array_equal(czy.distance_histogram(seven, 0.5, 400)[[1, 2, 4, 5, 6]], want)
    at = [0, 17, 150, 298, 299]
    big = filler.copy()
    big[at] = poses
    I, counts = czy.saxs(big, Q, 0.5, 400, counts=True)
    assert np.array_equal(counts[at], want)
    assert same_bits(I[at], czy.saxs(poses, Q, 0.5, 400))
    assert same_bits(I[[1, 2, 3]], czy.saxs(filler[[1, 2, 3]], Q, 0.5, 400))


def test_more_poses_than_a_chunk_holds(czy, ranked):
    poses, want = ranked
    seven = np.concatenate([poses, poses[:2]])
    for chunk in (1, 2, 3, 7, 100):
        assert np.array_equal(czy.distance_histogram(seven, 0.5, 400, chunk=chunk), np.concatenate([want, want[:2]]))
    whole = czy.saxs(seven, Q, 0.5, 400)
    I, counts = czy.saxs(seven, Q, 0.5, 400, counts=True, chunk=2)
    assert same_bits(I, whole) and np.array_equal(counts[:5], want)


def test_a_receptor_without_modes_equals_zero_amplitude_modes(pkg, ranked):
    """Without receptor modes the receptor's own pairs are counted once a call and every row starts from them; with modes
    of amplitude zero they are counted pose by pose.  Also on 1ppe, rigid on both sides, against the restatement."""
    poses, _ = ranked
    rec_nm, lig_nm = np.load(os.path.join(CZY, "lightdock_rec.nm.npy")), np.load(os.path.join(CZY, "lightdock_lig.nm.npy"))
    still = poses.copy()
    still[:, 7:17] = 0.0
    no_modes = pkg.Complex(REC, LIG, None, 0, lig_nm, 10)
    with_modes = pkg.Complex(REC, LIG, rec_nm, 10, lig_nm, 10)
    a = no_modes.distance_histogram(np.concatenate([still[:, :7], still[:, 17:]], axis=1), 0.5, 400)
    b = with_modes.distance_histogram(still, 0.5, 400)
    assert np.array_equal(a, b)
    rs = sx.czy_saxs()
    assert np.array_equal(b[:2], rs.batch(still[:2], 500, 400))
    from test_gpu_contacts import case_complex
    from conftest import case_paths
    _, d, r, l = case_paths("1ppe")
    cx, rs = case_complex(pkg, "1ppe"), sx.SaxsRestated(r, l)
    p = np.loadtxt(os.path.join(d, "initial_positions_0.dat"))[:2, :7]
    assert np.array_equal(cx.distance_histogram(p, 0.5, 400), rs.batch(p, 500, 400))


# ---- 5. the Debye sum, exactly ----------------------------------------------------------------------------------

def test_debye_on_synthetic_counts_bit_for_bit(pkg):
    pkg.init(0)
    rng = np.random.default_rng(12)
    for bins, w in ((1, 500), (37, 137), (400, 500), (780, 300), (781, 300), (1024, 2000)):   # 780 | 781: 64 KB of LDS
        counts = np.zeros((6, 21, bins), dtype=np.uint32)                     # row 0 stays zero
        counts[1, 7, bins // 2] = 0xFFFFFFFF                                  # a single full bin
        counts[2] = 0xFFFFFF00 + rng.integers(0, 256, (21, bins))             # every word near 2^32
        counts[3] = rng.integers(0, 2 ** 31, (21, bins))
        counts[4, :, ::3] = rng.integers(0, 5000, (21, len(range(0, bins, 3))))
        counts[5, 20, bins - 1] = 1
        n_e = np.array([65536, 0, 3, 40000, 1, 7], dtype=np.uint32)
        q = np.concatenate([Q, rng.uniform(0, 1, 70)])
        got = pkg.saxs_debye(counts, n_e, q, w / 1000.0)
        f, s = pkg.saxs_form_factors(q), pkg.saxs_sinc(q, w / 1000.0, bins)
        want = np.array([sx.debye(c, n_e, f, s) for c in counts])
        assert same_bits(got, want)
        assert np.isfinite(got).all() and same_bits(got[0], sx.debye(counts[0], n_e, f, np.zeros_like(s)))
    many_q = np.linspace(0, 1, 1024)
    got = pkg.saxs_debye(counts[3:5], n_e, many_q, 2.0)
    f, s = pkg.saxs_form_factors(many_q), pkg.saxs_sinc(many_q, 2.0, 1024)
    assert same_bits(got, np.array([sx.debye(c, n_e, f, s) for c in counts[3:5]]))


def test_saxs_is_the_debye_sum_of_its_own_counts(pkg, czy, czy_rs, ranked):
    poses, want = ranked
    I, counts = czy.saxs(poses, Q, 0.5, 400, counts=True)
    assert np.array_equal(counts, want) and I.shape == (5, len(Q))
    f, s = pkg.saxs_form_factors(Q), pkg.saxs_sinc(Q, 0.5, 400)
    assert same_bits(I, np.array([czy_rs.profile(c, f, s) for c in counts]))
    assert same_bits(I, pkg.saxs_debye(counts, czy_rs.n_e, Q, 0.5))
    assert same_bits(I, czy.saxs(poses, Q, 0.5, 400))
    # the restatement's own tables (math.exp, math.sin) differ from the library's by rounding at most
    mine = np.array([czy_rs.profile(c, sx.form_factors(Q), sx.sinc(Q, 500, 400)) for c in counts])
    assert np.abs(I - mine).max() <= OWN_TABLES_RTOL * np.abs(mine).max()


# ---- 6. the Debye sum, physically -------------------------------------------------------------------------------

def test_two_atoms_scatter_as_the_formula_says(pkg, two_atoms):
    cx, _ = two_atoms
    t = [(0, 0, 0), (1.3, 0, 0), (0, 3.749, 0), (0.3, 0.4, 0)]
    I = cx.saxs(rigid(t), Q, 0.5, 8)
    f, s = pkg.saxs_form_factors(Q), pkg.saxs_sinc(Q, 0.5, 8)
    for i, k in enumerate((0, 2, 7, 1)):
        for j in range(len(Q)):
            f1, f2 = f[j, 1], f[j, 3]
            assert I[i, j] == (f1 * f1 + f2 * f2) + ((2.0 * f1) * f2) * s[j, k]
    assert abs(I[0, 0] - (f[0, 1] + f[0, 3]) ** 2) < 1e-9 * I[0, 0]


def test_binning_moves_a_1czy_profile_by_less_than_the_derived_bound(czy, czy_rs, ranked):
    """|I_binned - I_direct| <= 2 sum_{a<b} |f_a f_b| 0.4362 q (w / 2000): 0.4362 bounds |d/dx sin(x) / x| and w / 2000 A is
    half a bin, the most a pair's distance is from its bin's centre.  q > 0: at q = 0 both sides are the same sum."""
    poses, _ = ranked
    q = np.array([0.01, 0.03, 0.1, 0.2, 0.3, 0.5])
    t = czy_rs.thousandths(poses[0])
    direct, weight = sx.direct(t, czy_rs.classes, q)
    for w, bins in ((500, 400), (2000, 100), (150, 1024)):
        binned = czy.saxs(poses[:1], q, w / 1000.0, bins)[0]
        bound = 2.0 * weight * 0.4362 * q * (w / 2000.0)
        print("w %d: |I_binned - I_direct| / bound = %s" % (w, np.abs(binned - direct) / bound))
        assert (np.abs(binned - direct) <= bound).all()


# ---- 7. refusals ------------------------------------------------------------------------------------------------

def raw_saxs(lib, cx, poses, width=500, bins=400, q=Q, n_q=None, stride=None, want=(True, True)):
    """ld_complex_saxs on buffers filled with 0xA5 -> (status, untouched)."""
    poses = np.ascontiguousarray(poses, dtype=np.float64)
    n = len(poses)
    q = None if q is None else np.ascontiguousarray(q, dtype=np.float64)
    n_q = (0 if q is None else len(q)) if n_q is None else n_q
    bufs = [np.full((n, max(1, min(n_q, 1024))), np.nan), np.full((n, 21, max(1, min(bins, 1024))), 0xA5A5A5A5, dtype=np.uint32)]
    bufs[0].view(np.uint8)[:] = FILL
    ptrs = [b.ctypes.data_as(ctypes.c_void_p) if w else None for b, w in zip(bufs, want)]
    status = lib.ld_complex_saxs(cx._h, n, poses.ctypes.data_as(ctypes.c_void_p), poses.shape[1] if stride is None else stride, width, bins,
                                 None if q is None else q.ctypes.data_as(ctypes.c_void_p), n_q, *ptrs)
    return status, all((b.view(np.uint8) == FILL).all() for b in bufs)


def test_refusals_by_status_with_the_outputs_untouched(pkg, czy, ranked, tmp_path):
    poses, want = ranked
    poses = poses[:3]
    lib = pkg.load_library()
    assert raw_saxs(lib, czy, poses) == (0, False)
    assert raw_saxs(lib, czy, poses, want=(False, False)) == (0, True) and raw_saxs(lib, czy, poses, want=(True, False))[0] == 0
    for kw in (dict(width=99), dict(width=2001), dict(width=0), dict(bins=0), dict(bins=1025), dict(q=Q, n_q=0), dict(q=np.full(1025, 0.1)),
               dict(q=None, n_q=3), dict(q=[0.1, -1e-9]), dict(q=[1.0000001]), dict(q=[0.1, float("nan")]), dict(q=[float("inf")]),
               dict(stride=26), dict(bins=40)):                                # 40 bins: a pair beyond the last
        assert raw_saxs(lib, czy, poses, **kw) == (-1, True), kw
        assert lib.ld_last_error().decode()
    for bad in (np.nan, np.inf, -np.inf):
        p = poses.copy()
        p[1, 12] = bad
        assert raw_saxs(lib, czy, p) == (-1, True)
    z = poses.copy()
    z[2, 3:7] = 0.0
    assert raw_saxs(lib, czy, z) == (-1, True)
    far = poses.copy()
    far[0, 1] = 1.1e6                                       # beyond the coordinate bound, and beyond every bin
    assert raw_saxs(lib, czy, far, width=2000, bins=1024) == (-1, True)
    assert lib.ld_complex_saxs(czy._h, 0, None, 27, 500, 400, Q.ctypes.data_as(ctypes.c_void_p), len(Q), None, None) == 0
    assert lib.ld_complex_distance_histogram(czy._h, 0, None, 27, 500, 400, None) == 0
    for kw in (dict(width=0.099), dict(width=2.001), dict(bins=0), dict(bins=1025)):
        with pytest.raises(pkg.LightdockError):
            czy.distance_histogram(poses, **{"width": 0.5, "bins": 400, **kw})
    # a complex of only zinc atoms, on either side a bead
    rec, lig = pair_of_files(tmp_path, atom(1, "ZN", "ZN", "A", 1, (0, 0, 0), "ZN", True),
                             atom(1, "ZN", "ZN", "B", 1, (0, 0, 0), "ZN", True) + atom(2, "BJ", "MMB", "B", 2, (1, 0, 0), "C", True))
    zn = pkg.Complex(rec, lig)
    assert list(zn.saxs_classes(0)) == [255] and list(zn.saxs_classes(1)) == [255, 255]
    assert raw_saxs(lib, zn, rigid([(1, 0, 0), (2, 0, 0)])) == (-1, True)
    with pytest.raises(pkg.LightdockError):
        zn.distance_histogram(rigid([(1, 0, 0)]), 0.5, 8)
    # ld_saxs_debye's own
    counts, n_e = np.zeros((2, 21, 8), dtype=np.uint32), np.ones(6, dtype=np.uint32)
    for call in (lambda: pkg.saxs_debye(counts, n_e, Q, 0.05), lambda: pkg.saxs_debye(counts, n_e, [1.5], 0.5), lambda: pkg.saxs_debye(counts, n_e, [], 0.5),
                 lambda: pkg.saxs_debye(np.zeros((2, 21, 1025), dtype=np.uint32), n_e, Q, 0.5)):
        with pytest.raises(pkg.LightdockError):
            call()
    assert pkg.saxs_debye(np.zeros((0, 21, 8), dtype=np.uint32), n_e, Q, 0.5).shape == (0, len(Q))


# ---- 8. saxs.py end to end --------------------------------------------------------------------------------------

def snapshot(root):
    out = {}
    for d, _, files in os.walk(root):
        if os.path.basename(d) == "saxs" and os.path.dirname(d) == str(root):
            continue
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = hashlib.sha256(open(p, "rb").read()).hexdigest()
    return out


def run_saxs(pkg, run, *args):
    script = os.path.join(os.path.dirname(pkg.__file__), "saxs.py")
    r = subprocess.run([sys.executable, script] + list(args), cwd=run, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout, open(os.path.join(run, "saxs", "rank_saxs.list")).read()


def test_saxs_tool_on_a_copy_of_the_1czy_run(pkg, czy_rs, tmp_path):
    entries = analyse_module().ranking(range(10), 100, base=CZY)
    chosen = 4
    q = np.arange(1, 65) / 128.0                            # dyadic: (q * 10) / 10 == q, so --unit nm reads the same numbers
    assert ((q * 10.0) / 10.0 == q).all()
    profile = czy_rs.profile(czy_rs.counts(entries[chosen][2], 500, 400), sx.form_factors(q), sx.sinc(q, 500, 400))
    run, curves = tmp_path / "run", tmp_path / "curves"
    shutil.copytree(CZY, run)
    os.makedirs(curves)
    (curves / "exp.dat").write_text("# q I sigma\n\n" + "".join("%.17g %.17g %.17g\n" % (a, i, 0.03 * i) for a, i in zip(q, profile)) + "0.75 1.0 1.0\n")
    (curves / "exp_nm.dat").write_text("".join("%.17g %.17g %.17g\n" % (a * 10.0, i, 0.03 * i) for a, i in zip(q, profile)))
    before = snapshot(run)
    out, text = run_saxs(pkg, run, "setup.json", "100", "--swarms", "0-9", "--curve", str(curves / "exp.dat"), "--profiles", "2")
    assert "11 models fitted to 64 points" in out
    lines = text.splitlines()
    assert lines[0].split() == ["Swarm", "Glowworm", "Scoring", "chi2", "scale", "Rg", "Dmax"] and len(lines) == 12
    first = lines[1].split()
    assert (int(first[0]), int(first[1])) == (entries[chosen][0], entries[chosen][1])
    assert float(first[3]) < 1e-20 and abs(float(first[4]) - 1.0) < 1e-9
    chi2 = [float(l.split()[3]) for l in lines[1:]]
    assert chi2 == sorted(chi2) and chi2[1] > 1e-6
    assert sorted((int(l.split()[0]), int(l.split()[1])) for l in lines[1:]) == sorted((e[0], e[1]) for e in entries)
    counts = czy_rs.counts(entries[chosen][2], 500, 400)
    H = counts.sum(axis=0).astype(np.float64)
    r = (np.arange(400) + 0.5) * 0.5
    assert first[5] == "%.3f" % math.sqrt((H * r * r).sum() / czy_rs.n_part ** 2) and first[6] == "%.3f" % ((np.flatnonzero(H)[-1] + 1) * 0.5)
    assert 10.0 < float(first[5]) < float(first[6]) < 200.0
    assert sorted(os.listdir(run / "saxs")) == ["profile_1.dat", "profile_2.dat", "rank_saxs.list"]
    rows = np.loadtxt(run / "saxs" / "profile_1.dat")
    assert rows.shape == (64, 4) and np.allclose(rows[:, 0], q, rtol=1e-8) and np.allclose(rows[:, 3], rows[:, 1], rtol=1e-7)
    assert snapshot(run) == before                           # nothing else in the run directory changes
    _, again = run_saxs(pkg, run, "setup.json", "100", "--swarms", "0-9", "--curve", str(curves / "exp_nm.dat"), "--unit", "nm", "--qmax", "0.5")
    assert again == text
