"""The collision cross-section on the MI355X (ld_complex_ccs, lightdock-rust_amd/ccs.py): every comparison
is exact equality of integer arrays with the int64 numpy restatement of tests/ccs_reference.py."""
import ctypes
import itertools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import ccs_reference as cr
from test_analysis_cpu import CZY, analyse_module, tool_module
from test_gpu_contacts import REC, LIG, gso

pytestmark = pytest.mark.gpu

FILL = 0xA5
_reference = {}


def restated(rs, pose, what=2, probe=1.0, cell=0.5):
    """The reference's 64 counts of one pose, computed once a module run."""
    key = (id(rs), np.asarray(pose, dtype=np.float64).tobytes(), what, probe, cell)
    if key not in _reference:
        _reference[key] = rs.ccs(pose, what, probe, cell)
    return _reference[key]


def assert_equal(got, rs, poses, what=2, probe=1.0, cell=0.5):
    want = np.array([restated(rs, p, what, probe, cell) for p in poses], dtype=np.int64).reshape(len(poses), 64)
    assert got["counts"].dtype == np.uint32 and got["sums"].dtype == np.uint64 and got["ccs"].dtype == np.float64
    assert got["counts"].shape == want.shape and got["sums"].shape == (len(poses),)
    assert np.array_equal(got["counts"], want)
    assert np.array_equal(got["sums"], want.sum(axis=1).astype(np.uint64))
    assert np.array_equal(got["ccs"], cr.ccs_pa(want.sum(axis=1), cell))
    return want


@pytest.fixture(scope="module")
def czy(pkg):
    pkg.init(0)
    return pkg.Complex(REC, LIG, np.load(os.path.join(CZY, "lightdock_rec.nm.npy")), 10, np.load(os.path.join(CZY, "lightdock_lig.nm.npy")), 10)


@pytest.fixture(scope="module")
def czy_rigid(pkg):
    pkg.init(0)
    return pkg.Complex(REC, LIG)


@pytest.fixture(scope="module")
def czy_rs():
    return cr.czy_ccs()


@pytest.fixture(scope="module")
def czy_rigid_rs():
    return cr.czy_ccs(modes=False)


@pytest.fixture(scope="module")
def ranked():
    """The first three ranked models of the golden run, (3, 27)."""
    entries = analyse_module().ranking(range(10), 100, base=CZY)
    return np.array([e[2] for e in entries[:3]])


def atom(serial, name, resname, chain, seq, xyz, element):
    return "ATOM  %5d %-4s %3s %1s%4d    %8.3f%8.3f%8.3f  1.00  0.00          %2s  \n" % ((serial, name, resname, chain, seq) + tuple(xyz) + (element,))


def pair_of_files(tmp_path, rec_text, lig_text, tag=""):
    rec, lig = tmp_path / ("rec%s.pdb" % tag), tmp_path / ("lig%s.pdb" % tag)
    rec.write_text(rec_text)
    lig.write_text(lig_text)
    return str(rec), str(lig)


def carbons(tmp_path, rec_xyz, lig_xyz, tag=""):
    rec = "".join(atom(i + 1, "C", "GLY", "A", i + 1, xyz, "C") for i, xyz in enumerate(rec_xyz))
    lig = "".join(atom(i + 1, "C", "GLY", "B", i + 1, xyz, "C") for i, xyz in enumerate(lig_xyz))
    return pair_of_files(tmp_path, rec, lig, tag)


def both_forms(pkg, rec, lig):
    """The same two files without modes (the rigid-receptor form) and with one all-zero mode a side (the plain form), and
    what turns a 7-column pose into a pose of each."""
    n_rec, n_lig = len(cr.sr.records(rec)), len(cr.sr.records(lig))
    return ((pkg.Complex(rec, lig), cr.CcsRestated(rec, lig), lambda p: p),
            (pkg.Complex(rec, lig, np.zeros(3 * n_rec), 1, np.zeros(3 * n_lig), 1),
             cr.CcsRestated(rec, lig, np.zeros((1, n_rec, 3)), np.zeros((1, n_lig, 3))), lambda p: np.hstack([p, np.zeros((len(p), 2))])))


def rigid(t):
    """Translations (n, 3) -> poses (n, 7) with the identity rotation."""
    t = np.asarray(t, dtype=np.float64).reshape(-1, 3)
    poses = np.zeros((len(t), 7))
    poses[:, :3], poses[:, 3] = t, 1.0
    return poses


# ---- 1. knife edges ---------------------------------------------------------------------------------------------

def test_knife_edges_of_two_atoms(pkg, tmp_path):
    """A one-atom receptor and a one-atom ligand, E = 2500 (C with probe 0.8) at h = 500; the pose moves the ligand in
    0.0005 A steps.  View 0 has A = (0, 2^20, 0): there a is the printed y itself, and b = 0 while x = z = 0."""
    pkg.init(0)
    assert cr.FRAMES[0].tolist() == [[0, 1048576, 0], [-1040384, 0, 130816]]
    k = 0.0005 * np.arange(41)
    zero = np.zeros(41)
    for sign in (1.0, -1.0):
        for origin, tag in (((0.0, 0.0, 0.0), "o"), ((-13.0, -7.5, -21.0), "n")):
            rec, lig = carbons(tmp_path, [origin], [(0.0, 0.0, 0.0)], tag + ("p" if sign > 0 else "m"))
            cx, rs = pkg.Complex(rec, lig), cr.CcsRestated(rec, lig)
            o = np.array(origin)
            sweeps = {"part": o + sign * np.stack([zero, 4.990 + k, zero], axis=1),          # the discs part in view 0 at 5.000
                      "rim": o + sign * np.stack([zero, 0.490 + k, zero], axis=1),           # lattice points on the rim at 0.500
                      "round": o + sign * np.stack([1.2340 + k, zero + 0.3, zero - 0.2], axis=1)}   # a of the oblique views steps
            for name, t in sweeps.items():
                poses = rigid(t)
                got = {what: cx.ccs(poses, what, 0.8, 0.5, views=True) for what in (0, 1, 2)}
                for what in (0, 1, 2):
                    assert_equal(got[what], rs, poses, what, 0.8, 0.5)
                assert (got[2]["counts"] != got[2]["counts"][0]).any(), name       # some count changes inside the sweep
                assert (got[0]["counts"] == got[0]["counts"][0]).all()              # the receptor does not move
            if tag == "o":
                y = cr.thousandths(sweeps["rim"][:, 1])
                lig0 = cx.ccs(rigid(sweeps["rim"]), 1, 0.8, 0.5, views=True)["counts"][:, 0]
                assert (lig0[np.abs(y) == 500] == 81).all() and (lig0[np.abs(y) == 499] < 81).all() and (lig0[np.abs(y) == 501] < 81).all()
                y = cr.thousandths(sweeps["part"][:, 1])
                all0 = cx.ccs(rigid(sweeps["part"]), 2, 0.8, 0.5, views=True)["counts"][:, 0]
                lig0 = cx.ccs(rigid(sweeps["part"]), 1, 0.8, 0.5, views=True)["counts"][:, 0]
                assert (all0[np.abs(y) == 5000] == 81 + 81 - 1).all() and (all0[np.abs(y) > 5000] == 81 + lig0[np.abs(y) > 5000]).all()
                assert (all0[np.abs(y) < 5000] < 81 + lig0[np.abs(y) < 5000]).all()
                a = cr.project(cr.thousandths(sweeps["round"]))[0][1]              # view 1: a = 0.675 x + ... steps on some thousandths only
                x = cr.thousandths(sweeps["round"][:, 0])
                assert 1 < len(set(a.tolist())) < len(set(x.tolist()))


# ---- 2. 1czy ----------------------------------------------------------------------------------------------------

def test_1czy_ranked_poses_with_modes_in_all_three_selections(czy, czy_rs, ranked):
    assert ranked.shape == (3, 27) and czy.pose_len == 27
    got = {what: czy.ccs(ranked, what, views=True) for what in (0, 1, 2)}
    want = {what: assert_equal(got[what], czy_rs, ranked, what) for what in (0, 1, 2)}
    assert (want[2] >= np.maximum(want[0], want[1])).all() and (want[2] <= want[0] + want[1]).all() and (want[2] < want[0] + want[1]).any()
    assert np.array_equal(czy.ccs(ranked)["sums"], got[2]["sums"]) and "counts" not in czy.ccs(ranked)
    print("1czy, first ranked model: CCS_PA complex %.1f, receptor %.1f, ligand %.1f A^2" % tuple(got[w]["ccs"][0] for w in (2, 0, 1)))
    for probe, cell in ((0.0, 0.5), (2.0, 2.0), (1.4, 0.333)):
        assert_equal(czy.ccs(ranked[:1], 2, probe, cell, views=True), czy_rs, ranked[:1], 2, probe, cell)


# ---- 3. batches -------------------------------------------------------------------------------------------------

def raw_call(lib, cx, poses, what=2, probe=1.0, cell=0.5, want=(True, True), stride=None):
    """ld_complex_ccs on buffers filled with 0xA5 -> (status, counts, sums) (None where not asked for)."""
    poses = np.ascontiguousarray(poses, dtype=np.float64)
    n = len(poses)
    bufs = [np.full((n, 64), 0xA5A5A5A5, dtype=np.uint32), np.full(n, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)]
    bufs = [b if w else None for b, w in zip(bufs, want)]
    ptrs = [None if b is None else b.ctypes.data_as(ctypes.c_void_p) for b in bufs]
    status = lib.ld_complex_ccs(cx._h, n, poses.ctypes.data_as(ctypes.c_void_p), poses.shape[1] if stride is None else stride, what,
                                ctypes.c_double(probe), ctypes.c_double(cell), *ptrs)
    return (status,) + tuple(bufs)


def untouched(bufs):
    return all(b is None or (b.view(np.uint8) == FILL).all() for b in bufs)


def test_batches_slots_strides_and_null_outputs(pkg, czy, czy_rs, ranked):
    want = np.array([restated(czy_rs, p) for p in ranked])
    # the same three poses at 1100 places, more than the 1024 slots, rows 30 doubles apart with NaN between them
    n = 1100
    source = (np.arange(n) * 7) % 3
    poses = np.full((n, 30), np.nan)
    poses[:, :27] = ranked[source]
    whole = czy.ccs(poses, views=True)
    print("1100 1czy poses: ccs kernel %.3f ms" % czy.last_kernel_ms())
    assert np.array_equal(whole["counts"], want[source].astype(np.uint32))
    assert np.array_equal(whole["sums"], want[source].sum(axis=1).astype(np.uint64))
    pieces = [czy.ccs(poses[a:b], views=True) for a, b in ((0, 1), (1, 1025), (1025, 1100))]
    for key in ("counts", "sums", "ccs"):
        assert np.concatenate([p[key] for p in pieces]).tobytes() == whole[key].tobytes()
    lib = pkg.load_library()
    for asked in itertools.product((False, True), repeat=2):
        status, counts, sums = raw_call(lib, czy, poses[:5], want=asked)
        assert status == 0
        assert counts is None or np.array_equal(counts, whole["counts"][:5])
        assert sums is None or np.array_equal(sums, whole["sums"][:5])
    empty = czy.ccs(np.zeros((0, 27)), views=True)
    assert empty["counts"].shape == (0, 64) and empty["sums"].shape == (0,) and empty["ccs"].shape == (0,)
    assert lib.ld_complex_ccs(czy._h, 0, None, 27, 2, ctypes.c_double(1.0), ctypes.c_double(0.5), None, None) == 0
    frames = pkg.ccs_frames()
    assert frames.dtype == np.int32 and np.array_equal(frames, cr.FRAMES)


# ---- 4. strips --------------------------------------------------------------------------------------------------

def test_boxes_beyond_the_bitmap_are_cut_into_pieces(pkg, czy, czy_rs, ranked, tmp_path):
    """At h = 100: two atoms 4000 A apart along z (e1 has no z component, so every view's box is 55 columns by up to 40 000
    rows: long and thin, and inside the 2^28 bound, which 4000 A along x or y are not), three atoms spread 600 A along each
    axis (boxes of 10^7 points and more), in the rigid-receptor and in the plain form, and a 1czy pose."""
    pkg.init(0)
    rec, lig = carbons(tmp_path, [(0, 0, 0)], [(0, 0, 0)], "two")
    for cx, rs, widen in both_forms(pkg, rec, lig):
        poses = widen(rigid([(0, 0, 4000.0), (0, 0, -4000.0), (0.3, -0.2, 2600.0), (-0.0005, 0.0015, -3999.9995)]))
        want = assert_equal(cx.ccs(poses, 2, 1.0, 0.1, views=True), rs, poses, 2, 1.0, 0.1)
        alone = restated(rs, poses[0], 0, 1.0, 0.1)
        assert np.array_equal(want[0], alone + restated(rs, poses[0], 1, 1.0, 0.1)) and alone.min() == alone.max() == cr.brute_count(np.array([0]), np.array([0]), np.array([2700]), 100)
    spread = [(0, 0, 0), (600.0, 600.0, 0), (0, 600.0, 600.0)]
    for k, (r, l) in enumerate(((spread[:2], spread[2:]), (spread[:1], spread[1:]))):
        rec, lig = carbons(tmp_path, r, l, "three%d" % k)
        for cx, rs, widen in both_forms(pkg, rec, lig):
            poses = widen(rigid([(0, 0, 0), (-0.25, 0.125, 600.0)]))
            t = cr.thousandths(rs.pose(poses[0]))
            a, b = cr.project(t)
            assert max(cr.box_points(a[v], b[v], np.full(3, 2700), 100) for v in range(64)) > 10 ** 7
            assert_equal(cx.ccs(poses, 2, 1.0, 0.1, views=True), rs, poses, 2, 1.0, 0.1)
    assert_equal(czy.ccs(ranked[:1], 2, 1.0, 0.1, views=True), czy_rs, ranked[:1], 2, 1.0, 0.1)


# ---- 5. the rigid-receptor form ---------------------------------------------------------------------------------

def test_rigid_receptor_form_gives_the_plain_form_bits(czy, czy_rigid, czy_rigid_rs, ranked):
    flat = ranked[:, :7].copy()
    fast = czy_rigid.ccs(flat, views=True)
    want = assert_equal(fast, czy_rigid_rs, flat)
    at_rest = np.hstack([flat, np.zeros((3, 20))])
    plain = czy.ccs(at_rest, views=True)
    for key in ("counts", "sums", "ccs"):
        assert plain[key].tobytes() == fast[key].tobytes()
    assert not np.array_equal(want, np.array([restated(czy_rigid_rs, p, 1) for p in flat]))
    for what in (0, 1):       # the selections of one side go the plain way in both
        assert_equal(czy_rigid.ccs(flat[:1], what, views=True), czy_rigid_rs, flat[:1], what)
        assert np.array_equal(czy.ccs(at_rest[:1], what, views=True)["counts"], czy_rigid.ccs(flat[:1], what, views=True)["counts"])
    far = flat.copy()
    far[1, :3] += (150.0, -80.0, 40.0)      # the ligand's box apart from the receptor's
    assert_equal(czy_rigid.ccs(far[1:2], views=True), czy_rigid_rs, far[1:2])


# ---- 6. refusals ------------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched(pkg, czy, czy_rigid, ranked, tmp_path):
    lib = pkg.load_library()

    def refused(cx, p, what=2, probe=1.0, cell=0.5, stride=None):
        out = raw_call(lib, cx, p, what, probe, cell, stride=stride)
        assert out[0] == -1 and lib.ld_last_error().decode()
        assert untouched(out[1:])

    for cx, poses in ((czy, ranked), (czy_rigid, ranked[:, :7])):
        for probe in (-0.001, -1.0, 2.001, float("nan"), float("inf"), -float("inf"), 1e300):
            refused(cx, poses, probe=probe)
            with pytest.raises(pkg.LightdockError):
                cx.ccs(poses, probe=probe)
        for cell in (0.0994, 0.0, -0.5, 2.0006, float("nan"), float("inf"), -float("inf"), 1e300):
            refused(cx, poses, cell=cell)
        for what in (-1, 3, 7):
            refused(cx, poses, what=what)
        for bad in (np.nan, np.inf, -np.inf):
            p = poses.copy()
            p[1, 5] = bad
            refused(cx, p)
        z = poses.copy()
        z[2, 3:7] = 0.0
        refused(cx, z)
        refused(cx, poses[:, :6])                  # stride below the pose length
        over = poses.copy()
        over[2, 2] = -1.1e6                        # beyond the coordinate bound, found by the kernel
        refused(cx, over)
        refused(cx, over, what=1)
        assert raw_call(lib, cx, over, what=0)[0] == 0          # the receptor alone does not move
        ok = raw_call(lib, cx, poses)
        assert ok[0] == 0 and not untouched(ok[1:])
    # no selected atom takes part
    rec, lig = pair_of_files(tmp_path, atom(1, "C", "GLY", "A", 1, (0, 0, 0), "C"),
                             atom(1, "H", "GLY", "B", 1, (0, 0, 0), "H") + atom(2, "BJ", "MMB", "B", 2, (1, 0, 0), "C"), "h")
    p = rigid([(0, 0, 0), (3.0, 0, 0)])
    for a, b, none in ((rec, lig, 1), (lig, rec, 0)):
        cx = pkg.Complex(a, b)
        refused(cx, p, what=none)
        for what in (1 - none, 2):
            status, counts, _ = raw_call(lib, cx, p, what, 0.8, 0.5)
            assert status == 0 and (counts[0] == 81).all()
    # the box bound at h = 100: the last translation along (1, 1, 0) whose largest box holds 2^28 points at most, and the next
    rec, lig = carbons(tmp_path, [(0, 0, 0)], [(0, 0, 0)], "box")
    E = np.array([2700, 2700])

    def largest_box(t):
        a, b = cr.project(np.array([[0, 0, 0], [t, t, 0]]))
        return max(cr.box_points(a[v], b[v], E, 100) for v in range(64))

    lo, hi = 1000000, 2000000                     # thousandths
    assert largest_box(lo) <= cr.MAX_BOX < largest_box(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if largest_box(mid) <= cr.MAX_BOX else (lo, mid)
    assert cr.MAX_BOX - 20000 < largest_box(lo) <= cr.MAX_BOX < largest_box(hi) < cr.MAX_BOX + 20000
    for cx, rs, widen in both_forms(pkg, rec, lig):
        inside, beyond = widen(rigid([(lo / 1000.0, lo / 1000.0, 0)])), widen(rigid([(hi / 1000.0, hi / 1000.0, 0)]))
        assert cr.thousandths(inside[0, 0]) == lo and cr.thousandths(beyond[0, 0]) == hi
        assert_equal(cx.ccs(inside, 2, 1.0, 0.1, views=True), rs, inside, 2, 1.0, 0.1)
        refused(cx, beyond, cell=0.1)
        refused(cx, np.vstack([inside, beyond, inside]), cell=0.1)
        assert raw_call(lib, cx, beyond, what=1, cell=0.1)[0] == 0        # the ligand alone: a small box


# ---- 7. the tool ------------------------------------------------------------------------------------------------

def run_tool(pkg, run, *args):
    script = os.path.join(os.path.dirname(pkg.__file__), "ccs.py")
    r = subprocess.run([sys.executable, script] + list(args), cwd=run, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout, open(os.path.join(run, "ccs", "rank_ccs.list")).read().splitlines()


def test_ccs_tool_on_a_copy_of_the_1czy_run(pkg, czy_rs, ranked, tmp_path):
    tool = tool_module("ccs")
    entries = analyse_module().ranking(range(10), 100, base=CZY)
    run = tmp_path / "run"
    shutil.copytree(CZY, run)
    out, lines = run_tool(pkg, run, "setup.json", "100", "--swarms", "0-9", "--top", "2")
    print(out.strip())
    assert "11 models measured" in out and len(lines) == 2 + 1 + 11
    for line, what, name in zip(lines[:2], (0, 1), ("receptor", "ligand")):
        ccs, lo, hi = tool.areas(restated(czy_rs, ranked[0], what), 500)
        assert line + "\n" == tool.monomer_text(name, ccs[0], lo[0], hi[0])
    assert lines[2] + "\n" == tool.HEADER
    for line, e, pose in zip(lines[3:6], entries, ranked):
        ccs, lo, hi = tool.areas(restated(czy_rs, pose), 500)
        assert line == "%5d %9d %11.5f %11.2f %9.2f %9.2f" % (e[0], e[1], e[3]["scoring"], ccs[0], lo[0], hi[0])
    assert [tuple(int(v) for v in l.split()[:2]) for l in lines[3:]] == [e[:2] for e in entries]        # the run's ranking is kept
    assert sorted(os.listdir(run / "ccs")) == ["model_1.pdb", "model_2.pdb", "rank_ccs.list"]
    measured = {tuple(int(v) for v in l.split()[:2]): float(l.split()[3]) for l in lines[3:]}
    X, K, S = 0.97 * float(np.median(list(measured.values()))), 0.98, 25.0
    out, exp = run_tool(pkg, run, "setup.json", "100", "--swarms", "0-9", "--experimental", "%.3f" % X, "--scale", str(K), "--sigma", str(S))
    X = float("%.3f" % X)
    assert exp[:2] == lines[:2] and exp[2] + "\n" == tool.HEADER_EXP and len(exp) == len(lines)
    rows = [l.split() for l in exp[3:]]
    keys = [(int(r[0]), int(r[1])) for r in rows]
    by_rank = {e[:2]: k for k, e in enumerate(entries)}
    want = sorted(measured, key=lambda m: (abs(K * measured[m] - X), by_rank[m]))
    gaps = sorted(abs(K * v - X) for v in measured.values())
    assert min(b - a for a, b in zip(gaps, gaps[1:])) > 0.02          # the printed CCS settles the order
    assert keys == want and keys != [e[:2] for e in entries]
    for r in rows:
        assert float(r[3]) == measured[(int(r[0]), int(r[1]))]
        assert abs(float(r[6]) - (K * float(r[3]) - X)) < 0.011 and abs(float(r[7]) - float(r[6]) / S) < 0.0011
