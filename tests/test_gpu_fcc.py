"""Clustering by common contacts on the MI355X (ld_complex_pair_contacts, ld_fcc_common, ld_fcc_cluster,
ld_complex_cluster_fcc, lightdock-rust_amd/fcc.py): every comparison is exact equality with the int64 numpy
restatement of tests/fcc_reference.py."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import fcc_reference as ref
from test_analysis_cpu import CZY, tool_module
from test_contacts_cpu import GOLDEN, case_restated
from test_gpu_contacts import case_complex

pytestmark = pytest.mark.gpu

VP = ctypes.c_void_p


@pytest.fixture(scope="module")
def czy(pkg):
    pkg.init(0)
    return pkg.Complex(os.path.join(CZY, "lightdock_1czy_protein.pdb"), os.path.join(CZY, "lightdock_1czy_peptide.pdb"),
                       np.load(os.path.join(CZY, "lightdock_rec.nm.npy")), 10, np.load(os.path.join(CZY, "lightdock_lig.nm.npy")), 10)


def ptr(a):
    return None if a is None else a.ctypes.data_as(VP)


# ---- 1. the free entries on random sets -------------------------------------------------------------------------------

def random_sets(seed, n, universe):
    """n strictly ascending sets over the given distinct keys: sizes from 0 to the whole universe, some sets empty, some the
    whole universe, some copies of an earlier one."""
    rng = np.random.default_rng(seed)
    universe = np.sort(np.asarray(universe, dtype=np.int64))
    U = len(universe)
    sets = []
    for i in range(n):
        kind = rng.integers(0, 8)
        if kind == 0:
            s = np.zeros(0, dtype=np.int64)
        elif kind == 1:
            s = universe.copy()
        elif kind == 2 and sets:
            s = sets[rng.integers(0, len(sets))].copy()
        elif kind == 3 and sets:                        # an earlier set and a few keys more or fewer: near a threshold
            flip = rng.random(U) < 2.0 / max(2, U)
            s = universe[np.isin(universe, sets[rng.integers(0, len(sets))]) ^ flip]
        else:
            s = universe[rng.random(U) < rng.random()]
        sets.append(s)
    offsets, keys = ref.to_csr(sets)
    scoring = np.round(rng.normal(0, 2, n), 1)          # ties in scoring
    return offsets, keys, scoring


def spread(seed, U, lo, hi):
    """U distinct keys of [lo, hi], both ends among them."""
    rng = np.random.default_rng(seed)
    keys = {lo, hi} if U > 1 else {hi}
    while len(keys) < U:
        keys.add(int(rng.integers(lo, hi + 1)))
    return sorted(keys)


SHAPES = [(1, range(1)), (2, range(7, 38)), (63, range(32)), (64, range(100, 133)), (65, spread(1, 64, 5, 90000)),
          (129, spread(2, 65, 0, 3000)), (257, spread(3, 4097, 1000, 70000)), (65, 2 ** 32 - 1 - np.arange(33)),
          (64, spread(4, 31, 0, 2 ** 32 - 1)), (257, range(1))]


def assert_cluster_equal(got, want):
    assert got["n_clusters"] == want["n_clusters"]
    for k in ("cluster_of", "centres", "set_sizes", "consensus"):
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), want[k]), k


@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_common_and_clusters_of_random_sets(pkg, case):
    pkg.init(0)
    n, universe = SHAPES[case]
    offsets, keys, scoring = random_sets(100 + case, n, universe)
    sizes = np.diff(offsets)
    assert n < 8 or (sizes.min() == 0 and sizes.max() == len(universe))
    want_c = ref.common(offsets, keys)
    got_c = pkg.fcc_common(offsets, keys)
    assert got_c.shape == (n, n) and np.array_equal(got_c.astype(np.int64), want_c)
    assert np.array_equal(np.diag(got_c), sizes)
    for threshold, min_size in ((0.6, 1), (0.001, 1), (1.0, 1), (0.5, 4), (0.75, n + 1)):
        want = ref.cluster(offsets, keys, scoring, threshold, min_size)
        got = pkg.fcc_cluster(offsets, keys, scoring, threshold, min_size)
        assert_cluster_equal(got, want)
        done = got["cluster_of"] >= 0
        counts = np.bincount(got["cluster_of"][done], minlength=got["n_clusters"])
        assert (np.diff(counts) <= 0).all() and (counts >= min_size).all()
        if min_size == n + 1:
            assert got["n_clusters"] == 0 and not done.any() and (got["centres"] == -1).all()
    assert pkg.fcc_last_kernel_ms() > 0.0


def test_a_pair_on_the_threshold_and_one_key_short_of_it(pkg):
    """s = 5 and 3 keys shared at T = 600: 1000 * 3 == 600 * 5 joins; with s = 6 on one side, 3000 < 3600 does not."""
    pkg.init(0)
    on = ref.to_csr([[1, 2, 3, 4, 5], [3, 4, 5, 8, 9]])
    short = ref.to_csr([[1, 2, 3, 4, 5], [3, 4, 5, 8, 9, 10]])
    score = np.array([0.0, 1.0])
    got = pkg.fcc_cluster(on[0], on[1], score, 0.6, 1)
    assert got["n_clusters"] == 1 and list(got["cluster_of"]) == [0, 0] and list(got["centres"]) == [1, -1]
    got = pkg.fcc_cluster(short[0], short[1], score, 0.6, 1)
    assert got["n_clusters"] == 2 and list(got["cluster_of"]) == [1, 0] and list(got["centres"]) == [1, 0]


# ---- 2. pair sets of the golden complexes -------------------------------------------------------------------------------

def assert_sets_equal(got, want):
    assert np.array_equal(got[0].astype(np.int64), want[0]) and np.array_equal(got[1].astype(np.int64), want[1])


def assert_projection_is_contacts(cx, poses, cutoff, sets=None):
    offsets, keys = cx.pair_contacts(poses, cutoff) if sets is None else sets
    rec, lig = ref.projection(offsets.astype(np.int64), keys.astype(np.int64), cx.num_residues(0), cx.num_residues(1))
    bits = cx.contacts(poses, cutoff)
    assert np.array_equal(rec, bits["rec"]) and np.array_equal(lig, bits["lig"])


def test_1azp_final_swarm(pkg):
    poses, scoring, _, offsets, keys, rs = ref.run_sets("1azp", 1)
    cx = case_complex(pkg, "1azp")
    got = cx.pair_contacts(poses[:, :cx.pose_len])
    assert_sets_equal(got, (offsets, keys))
    sizes = np.diff(offsets)
    assert (len(poses), sizes.min(), int(np.median(sizes)), sizes.max(), len(np.unique(keys))) == (200, 5, 22, 47, 144)
    for cutoff in (3.0, 5.0):
        assert_projection_is_contacts(cx, poses[:, :cx.pose_len], cutoff, got if cutoff == 5.0 else None)
    want = ref.cluster(offsets, keys, scoring, 0.6, 1)
    assert want["n_clusters"] == 11
    assert_cluster_equal(cx.cluster_fcc(poses[:, :cx.pose_len], scoring), want)
    assert_cluster_equal(pkg.fcc_cluster(got[0], got[1], scoring, 0.6, 1), want)


def test_1czy_three_swarms_with_modes_on_both_sides(pkg, czy):
    poses, scoring, _, offsets, keys, rs = ref.run_sets("1czy", 3)
    assert poses.shape == (600, 27)
    got = czy.pair_contacts(poses)
    assert_sets_equal(got, (offsets, keys))
    for cutoff in (3.0, 5.0):
        assert_projection_is_contacts(czy, poses, cutoff, got if cutoff == 5.0 else None)
    short = czy.pair_contacts(poses[:40], 3.0)
    assert_sets_equal(short, ref.pair_sets(rs, poses[:40], 3.0))
    for threshold, min_size in ((0.6, 1), (0.75, 3)):
        want = ref.cluster(offsets, keys, scoring, threshold, min_size)
        assert_cluster_equal(czy.cluster_fcc(poses, scoring, 5.0, threshold, min_size), want)
        assert_cluster_equal(pkg.fcc_cluster(got[0], got[1], scoring, threshold, min_size), want)
    assert czy.last_kernel_ms() > 0.0


@pytest.mark.parametrize("name,count", [("ab_icode", 48), ("1k4c", 32)])
def test_start_poses_give_empty_and_non_empty_sets(pkg, name, count):
    rs = case_restated(name)
    cx = case_complex(pkg, name)
    poses = np.loadtxt(os.path.join(GOLDEN, name, "initial_positions_0.dat"))[:count, :cx.pose_len]
    if name == "1k4c":          # every start pose of 1k4c touches the membrane: two of them again, 400 A away from it
        poses = np.concatenate([poses, poses[:2] + np.array([400.0] + [0.0] * (cx.pose_len - 1))])
    want = ref.pair_sets(rs, poses)
    got = cx.pair_contacts(poses)
    assert_sets_equal(got, want)
    sizes = np.diff(want[0])
    print("%s: %d poses, set sizes %d ... %d, %d empty" % (name, len(poses), sizes.min(), sizes.max(), (sizes == 0).sum()))
    assert (sizes == 0).any() and (sizes > 0).any()
    assert_projection_is_contacts(cx, poses, 5.0, got)
    assert_projection_is_contacts(cx, poses, 3.0)
    scoring = -np.arange(len(poses), dtype=np.float64)
    assert_cluster_equal(cx.cluster_fcc(poses, scoring), ref.cluster(want[0], want[1], scoring, 0.6, 1))


def test_a_pose_has_the_same_keys_in_any_batch(czy):
    """One pose alone, seven, and all 2000 final glowworms: more poses than the 1024 workspace slots."""
    poses, scoring, _, offsets, keys, _ = ref.run_sets("1czy", 10)
    whole = czy.pair_contacts(poses)
    assert_sets_equal(whole, (offsets, keys))
    sets = ref.from_csr(offsets, keys)
    for first, count in ((0, 1), (1999, 1), (1021, 7), (1100, 64)):
        o, k = czy.pair_contacts(poses[first:first + count])
        assert [list(s) for s in ref.from_csr(o.astype(np.int64), k)] == [list(s) for s in sets[first:first + count]]
    # the counts tests/test_fcc_cpu.py pins for the restatement; every word at the defaults
    for threshold, clusters, largest in ((0.5, 79, 169), (0.6, 95, 137), (0.75, 112, 127)):
        got = czy.cluster_fcc(poses, scoring, 5.0, threshold, 1)
        if threshold == 0.6:
            print("2000 final 1czy glowworms: cluster_fcc %.3f ms" % czy.last_kernel_ms())
            assert_cluster_equal(got, ref.run_clusters("1czy", 10))
        assert got["n_clusters"] == clusters and np.bincount(got["cluster_of"]).max() == largest


# ---- 3. the count protocol, caps, refusals --------------------------------------------------------------------------

MARK32, MARK64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5


def test_count_protocol_and_a_cap_too_small(pkg, czy):
    lib = pkg.load_library()
    poses, _, _, offsets, keys, _ = ref.run_sets("1czy", 3)
    p = np.ascontiguousarray(poses[:50])
    want_total = int(offsets[50])
    o = np.full(51, MARK32, dtype=np.uint32)
    total = ctypes.c_size_t(7)
    assert lib.ld_complex_pair_contacts(czy._h, 50, ptr(p), 27, ctypes.c_double(5.0), ptr(o), None, 0, ctypes.byref(total)) == 0
    assert total.value == want_total and np.array_equal(o.astype(np.int64), offsets[:51])
    total = ctypes.c_size_t(7)
    assert lib.ld_complex_pair_contacts(czy._h, 50, ptr(p), 27, ctypes.c_double(5.0), None, None, 0, ctypes.byref(total)) == 0
    assert total.value == want_total
    k = np.full(want_total + 3, MARK32, dtype=np.uint32)
    assert lib.ld_complex_pair_contacts(czy._h, 50, ptr(p), 27, ctypes.c_double(5.0), None, ptr(k), k.size, None) == 0
    assert np.array_equal(k[:want_total].astype(np.int64), keys[:want_total]) and (k[want_total:] == MARK32).all()
    for cap in (0, want_total - 1):
        o[:], k[:], total.value = MARK32, MARK32, 7
        assert lib.ld_complex_pair_contacts(czy._h, 50, ptr(p), 27, ctypes.c_double(5.0), ptr(o), ptr(k), cap, ctypes.byref(total)) == -1
        assert "room for" in lib.ld_last_error().decode()
        assert (o == MARK32).all() and (k == MARK32).all() and total.value == 7
    o[:], total.value = MARK32, 7
    assert lib.ld_complex_pair_contacts(czy._h, 0, None, 27, ctypes.c_double(5.0), ptr(o), None, 0, ctypes.byref(total)) == 0
    assert o[0] == 0 and (o[1:] == MARK32).all() and total.value == 0
    empty = czy.pair_contacts(np.zeros((0, 27)))
    assert list(empty[0]) == [0] and len(empty[1]) == 0


def test_refusals_of_the_complex_entries(pkg, czy):
    lib = pkg.load_library()
    poses, scoring, _, _, _, _ = ref.run_sets("1czy", 3)
    good, score = np.ascontiguousarray(poses[:6]), np.ascontiguousarray(scoring[:6])

    def refused(p=good, stride=27, s=score, cutoff=5.0, threshold=0.6, min_size=1, n=6, h=czy._h, pair=True):
        o, k = np.full(n + 1 if n < 100 else 7, MARK32, dtype=np.uint32), np.full(4096, MARK32, dtype=np.uint32)
        total = ctypes.c_size_t(7)
        a = lib.ld_complex_pair_contacts(h, n, ptr(p), stride, ctypes.c_double(cutoff), ptr(o), ptr(k), k.size, ctypes.byref(total)) if pair else -1
        pair_ok = a == -1 and (o == MARK32).all() and (k == MARK32).all() and total.value == 7
        m = 6 if n > 100 else n
        cl, ce = np.full(m, -7, dtype=np.int32), np.full(m, -7, dtype=np.int32)
        nc, ss, co = np.full(1, MARK32, dtype=np.uint32), np.full(m, MARK32, dtype=np.uint32), np.full(m, MARK64, dtype=np.uint64)
        b = lib.ld_complex_cluster_fcc(h, n, ptr(p), stride, ptr(s), ctypes.c_double(cutoff), ctypes.c_double(threshold), min_size,
                                       ptr(cl), ptr(ce), ptr(nc), ptr(ss), ptr(co))
        untouched = (cl == -7).all() and (ce == -7).all() and nc[0] == MARK32 and (ss == MARK32).all() and (co == MARK64).all()
        return pair_ok, b == -1 and untouched and bool(lib.ld_last_error().decode())

    for bad in (np.nan, np.inf):
        p = good.copy()
        p[2, 5] = bad
        assert refused(p=p) == (True, True)
    z = good.copy()
    z[1, 3:7] = 0.0
    assert refused(p=z) == (True, True)
    assert refused(p=np.ascontiguousarray(good[:, :20]), stride=20) == (True, True)
    far = good.copy()
    far[3, 0] = 1.1e6
    assert refused(p=far) == (True, True)
    for cutoff in (30.001, 0.0, -1.0, float("nan"), 1e300):
        assert refused(cutoff=cutoff) == (True, True)
    assert refused(h=None) == (True, True)
    assert refused(p=None) == (True, True)
    # an absurd n, before the list is read
    assert refused(n=2 ** 40) == (True, True)
    assert refused(n=65537, pair=False)[1]          # 65537 poses are a list ld_complex_pair_contacts takes
    # the clustering's own arguments
    for threshold in (float("nan"), 0.0, 0.0004, 1.0006, -0.5, 1e300, float("inf")):
        assert refused(threshold=threshold)[1]
    assert refused(min_size=0)[1]
    for bad in (np.nan, -np.inf):
        s = score.copy()
        s[4] = bad
        assert refused(s=s)[1]
    assert refused(s=None)[1]
    # and nothing was wrong with the list
    ok = czy.cluster_fcc(good, score)
    assert ok["n_clusters"] >= 1 and (ok["cluster_of"] >= 0).all()
    nc = np.full(1, MARK32, dtype=np.uint32)
    assert lib.ld_complex_cluster_fcc(czy._h, 0, None, 27, None, ctypes.c_double(5.0), ctypes.c_double(0.6), 1, None, None, ptr(nc), None, None) == 0
    assert nc[0] == 0
    # set_sizes and consensus are optional
    cl, ce = np.full(6, -7, dtype=np.int32), np.full(6, -7, dtype=np.int32)
    assert lib.ld_complex_cluster_fcc(czy._h, 6, ptr(good), 27, ptr(score), ctypes.c_double(5.0), ctypes.c_double(0.6), 1, ptr(cl), ptr(ce),
                                      ptr(nc), None, None) == 0
    assert np.array_equal(cl, ok["cluster_of"]) and np.array_equal(ce, ok["centres"]) and nc[0] == ok["n_clusters"]


def test_refusals_of_the_entries_that_take_sets(pkg):
    lib = pkg.load_library()
    pkg.init(0)
    offsets = np.array([0, 3, 3, 5], dtype=np.uint32)
    keys = np.array([2, 5, 9, 5, 4000000000], dtype=np.uint32)
    score = np.array([1.0, 2.0, 3.0])

    def refused(o=offsets, k=keys, s=score, threshold=0.6, min_size=1, n=3, both=True):
        m = 3 if n > 100 else n
        cl, ce = np.full(m, -7, dtype=np.int32), np.full(m, -7, dtype=np.int32)
        nc, co = np.full(1, MARK32, dtype=np.uint32), np.full(m, MARK64, dtype=np.uint64)
        a = lib.ld_fcc_cluster(n, ptr(o), ptr(k), ptr(s), ctypes.c_double(threshold), min_size, ptr(cl), ptr(ce), ptr(nc), ptr(co))
        ok = a == -1 and (cl == -7).all() and (ce == -7).all() and nc[0] == MARK32 and (co == MARK64).all()
        if both:
            c = np.full((m, m), MARK32, dtype=np.uint32)
            ok = ok and lib.ld_fcc_common(n, ptr(o), ptr(k), ptr(c)) == -1 and (c == MARK32).all()
        return ok and bool(lib.ld_last_error().decode())

    assert refused(o=np.array([0, 3, 2, 5], dtype=np.uint32))                      # offsets that do not ascend
    assert refused(o=np.array([1, 3, 3, 5], dtype=np.uint32))                      # or do not start at 0
    assert refused(k=np.array([2, 5, 5, 5, 9], dtype=np.uint32))                   # a key twice
    assert refused(k=np.array([2, 9, 5, 5, 9], dtype=np.uint32))                   # descending
    assert refused(o=None) and refused(k=None)
    assert refused(n=2 ** 40)                                                       # before anything is read
    assert refused(n=65537, both=False)
    for threshold in (float("nan"), 0.0, 1.0006, -1.0):
        assert refused(threshold=threshold, both=False)
    assert refused(min_size=0, both=False)
    assert refused(s=np.array([1.0, np.nan, 3.0]), both=False) and refused(s=None, both=False)
    got = pkg.fcc_cluster(offsets, keys, score, 0.5, 1)
    assert_cluster_equal(got, ref.cluster(offsets, keys, score, 0.5, 1))
    nc = np.full(1, MARK32, dtype=np.uint32)
    assert lib.ld_fcc_cluster(0, None, None, None, ctypes.c_double(0.6), 1, None, None, ptr(nc), None) == 0 and nc[0] == 0
    assert lib.ld_fcc_common(0, None, None, None) == 0
    # consensus is optional
    cl, ce = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32)
    assert lib.ld_fcc_cluster(3, ptr(offsets), ptr(keys), ptr(score), ctypes.c_double(0.5), 1, ptr(cl), ptr(ce), ptr(nc), None) == 0
    assert np.array_equal(cl, got["cluster_of"]) and nc[0] == got["n_clusters"]


# ---- 4. fcc.py end to end ---------------------------------------------------------------------------------------------

def test_fcc_tool_on_a_copy_of_the_1czy_run(pkg, czy, tmp_path):
    tool = tool_module("fcc")
    poses, scoring, entries, offsets, keys, _ = ref.run_sets("1czy", 10)
    want = ref.run_clusters("1czy", 10)
    run = tmp_path / "run"
    shutil.copytree(CZY, run)
    before = {f for f in os.listdir(run)}
    script = os.path.join(os.path.dirname(pkg.__file__), "fcc.py")
    r = subprocess.run([sys.executable, script, "setup.json", "100", "--all", "--top", "2"], cwd=run, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "2000 candidates: 95 clusters, 2 models written" in r.stdout
    assert sorted(os.listdir(run / "fcc")) == ["cluster_1.pdb", "cluster_2.pdb", "members.list", "rank_fcc.list"]
    assert {f for f in os.listdir(run)} == before | {"fcc"}
    assert (run / "fcc" / "rank_fcc.list").read_text() == tool.rank_fcc_text(entries, want["cluster_of"], want["centres"], want["n_clusters"])
    fraction = ref.consensus_fraction(want["consensus"], want["set_sizes"])
    assert (run / "fcc" / "members.list").read_text() == tool.members_text(entries, want["cluster_of"], want["set_sizes"], fraction)
    for c in (1, 2):
        path = str(tmp_path / "want.pdb")
        czy.write_pdb(poses[want["centres"][c - 1]], path)
        assert (run / "fcc" / ("cluster_%d.pdb" % c)).read_bytes() == open(path, "rb").read()
