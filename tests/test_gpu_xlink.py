"""The cross-links on the MI355X (ld_complex_crosslinks, lightdock-rust_amd/xlinks.py): every comparison is
exact equality of integer arrays with the numpy restatement of tests/xlink_reference.py."""
import ctypes
import itertools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import xlink_reference as xr
from test_analysis_cpu import CZY, analyse_module, tool_module
from test_gpu_ccs import atom, pair_of_files, rigid
from test_gpu_contacts import REC, LIG

pytestmark = pytest.mark.gpu

FILL = 0xA5
NONE = xr.NO_PATH
FAR = np.array([900000.0, -900000.0, 900000.0])
_reference = {}


def restated(rs, pose, links, **kw):
    """The restatement's (straight2, path) of one pose, computed once a module run."""
    key = (rs.tag, np.asarray(pose, dtype=np.float64).tobytes(), tuple(map(tuple, links)), tuple(sorted(kw.items())))
    if key not in _reference:
        _reference[key] = rs.crosslinks(pose, links, **kw)
    return _reference[key]


def wanted(rs, poses, links, **kw):
    got = [restated(rs, p, links, **kw) for p in poses]
    return (np.array([g[0] for g in got], dtype=np.uint64).reshape(len(poses), len(links)),
            np.array([g[1] for g in got], dtype=np.uint32).reshape(len(poses), len(links)))


def assert_equal(cx, rs, poses, links, **kw):
    """cx.crosslinks against the restatement -> (straight2 (n, L) as int64, path (n, L) as int64)."""
    got = cx.crosslinks(poses, links, **kw)
    straight2, path = wanted(rs, poses, links, **kw)
    assert got["straight2"].dtype == np.uint64 and got["path"].dtype == np.uint32 and got["straight"].dtype == np.float64
    assert got["straight2"].shape == got["path"].shape == got["straight"].shape == (len(poses), len(links))
    assert np.array_equal(got["straight2"], straight2)
    assert np.array_equal(got["path"], path)
    assert np.array_equal(got["straight"], np.sqrt(straight2.astype(np.float64)) / 1000.0)
    return straight2.astype(np.int64), path.astype(np.int64)


def field(v):
    """A coordinate in the 8 columns of a PDB record: "%8.3f" where that fits, else fewer decimals (900001.5, -900006.)."""
    s = "%8.3f" % v
    while len(s) > 8 and s[-1] in "0.":
        s = s[:-1]
    assert len(s) <= 8 and float(s) == v, v
    return "%8s" % s


def record(serial, name, resname, chain, seq, xyz, element):
    return "ATOM  %5d %-4s %3s %1s%4d    %s%s%s  1.00  0.00          %2s  \n" % ((serial, name, resname, chain, seq) + tuple(field(v) for v in xyz) + (element,))


def molecule(atoms, chain, shift=(0.0, 0.0, 0.0)):
    """atoms: [(element, (x, y, z))] -> the text of a PDB file, one residue an atom."""
    return "".join(record(i + 1, e, "GLY", chain, i + 1, np.asarray(xyz, dtype=np.float64) + np.asarray(shift), e) for i, (e, xyz) in enumerate(atoms))


def both(pkg, tmp_path, rec_atoms, lig_atoms, tag, shift=(0.0, 0.0, 0.0)):
    rec, lig = pair_of_files(tmp_path, molecule(rec_atoms, "A", shift), molecule(lig_atoms, "B"), tag)
    rs = xr.XlinkRestated(rec, lig)
    rs.tag = (tag, tuple(shift))             # what restated() knows it by: a tag names one pair of files
    return pkg.Complex(rec, lig), rs


@pytest.fixture(scope="module")
def czy(pkg):
    pkg.init(0)
    return pkg.Complex(REC, LIG, np.load(os.path.join(CZY, "lightdock_rec.nm.npy")), 10, np.load(os.path.join(CZY, "lightdock_lig.nm.npy")), 10)


@pytest.fixture(scope="module")
def czy_rs():
    rs = xr.czy_xlink()
    rs.tag = "1czy"
    return rs


@pytest.fixture(scope="module")
def ranked():
    """The first three ranked models of the golden run, (3, 27)."""
    entries = analyse_module().ranking(range(10), 100, base=CZY)
    return np.array([e[2] for e in entries[:3]])


def czy_links(rs):
    """Eight links between CA atoms by a fixed rule.  With r the receptor's CA atoms and l the ligand's, in file order and
    n = len(r): between the molecules (r[0], l[0]) and (r[n / 2], l[len(l) / 2]); inside the receptor (r[0], r[2]) and
    (r[0], r[4]) -- with the first, three that share an anchor --, (r[n / 2], r[n / 2 + 6]), (r[n / 4], r[n / 4 + 5]) and
    (r[-1], r[-7]); inside the ligand (l[0], l[-1])."""
    names = [[line[12:16].strip() for line in xr.sr.records(path)] for path in (REC, LIG)]
    r = [k for k, name in enumerate(names[0]) if name == "CA"]
    l = [len(names[0]) + k for k, name in enumerate(names[1]) if name == "CA"]
    n = len(r)
    assert n >= 16 and len(l) >= 4 and len(names[0]) == rs.n_rec
    return [(r[0], l[0]), (r[n // 2], l[len(l) // 2]), (r[0], r[2]), (r[0], r[4]), (r[n // 2], r[n // 2 + 6]), (r[n // 4], r[n // 4 + 5]), (r[-1], r[-7]),
            (l[0], l[-1])]


# ---- 1. knife edges ---------------------------------------------------------------------------------------------

CASES = [(sign, origin, tag) for sign in (1.0, -1.0) for origin, tag in (((0.0, 0.0, 0.0), "o"), ((-13.0, -7.5, -21.0), "n"))]


@pytest.mark.parametrize("sign,origin,tag", CASES)
def test_knife_edges_of_tiny_files(pkg, tmp_path, sign, origin, tag):
    """Files of a few atoms about `origin`, mirrored by `sign`; the pose moves the ligand in 0.0005 A steps.  h = 1000,
    max_length 12: boxes of 25^3 at most.  The values the text pins are asserted where the origin is a lattice node."""
    pkg.init(0)
    o, k, zero = np.array(origin), 0.0005 * np.arange(41), np.zeros(41)
    tag += "p" if sign > 0 else "m"
    at_node = tag[0] == "o"
    kw = dict(max_length=12.0)

    # two carbons and nothing between, 9.990 .. 10.010 A apart
    cx, rs = both(pkg, tmp_path, [("C", o)], [("C", (0, 0, 0))], "two" + tag)
    poses = rigid(o + sign * np.stack([9.990 + k, zero, zero], axis=1))
    links = [(0, 1), (1, 0), (0, 0), (1, 1)]
    straight2, path = assert_equal(cx, rs, poses, links, **kw)
    assert len(set(straight2[:, 0].tolist())) > 10 and len(set(path[:, 0].tolist())) > 10         # values change inside the sweep
    assert np.array_equal(path[:, 0], path[:, 1]) and (straight2[:, 2:] == 0).all()
    if at_node:
        x = np.abs(xr.thousandths(poses[:, 0]))
        assert np.array_equal(straight2[:, 0], x * x)
        # at 10.000 the doors (2, 0, 0) and (8, 0, 0), two hops of 2000 and six moves; about a lone carbon the door (1, 1, 1)
        assert (path[x == 10000, 0] == 10000).all() and (path[x == 10000, 2] == 2 * 1732).all()
        # D == M is reported, D == M + 1 is not
        at = poses[x == 10000][:1]
        assert assert_equal(cx, rs, at, links, max_length=10.0)[1][0].tolist() == [10000, 10000, 3464, 3464]
        assert assert_equal(cx, rs, at, links, max_length=9.999)[1][0].tolist() == [NONE, NONE, 3464, 3464]

    # one blocker on the lattice line between two anchors that block nothing, moved across the line: the node (4, 0, 0) is
    # blocked while the carbon's centre is less than 1700 from it, strictly
    cx, rs = both(pkg, tmp_path, [("H", o), ("H", o + sign * np.array([8.0, 0, 0]))], [("C", (0, 0, 0))], "rim" + tag)
    poses = rigid(o + sign * np.stack([zero + 4.0, 1.690 + k, zero], axis=1))
    straight2, path = assert_equal(cx, rs, poses, [(0, 1), (1, 0), (0, 2)], **kw)
    assert (straight2[:, 0] == 64000000).all() and np.array_equal(path[:, 0], path[:, 1])
    if at_node:
        y = np.abs(xr.thousandths(poses[:, 1]))
        assert (y == 1699).any() and (y == 1700).any()
        assert (path[y < 1700, 0] > 8000).all() and (path[y >= 1700, 0] == 8000).all()            # D steps exactly there

    # a door at exactly rho: a hydrogen x from the node (0, 0, 0) with a reach of 0.5 A, the node (1, 0, 0) blocked by a
    # carbon 1600 beyond it: the node at 500 is a door, at 501 it is not and the anchor has none -- its straight distances
    # are given all the same
    cx, rs = both(pkg, tmp_path, [("C", o + sign * np.array([2.6, 0, 0]))], [("H", (0, 0, 0))], "door" + tag)
    poses = rigid(o + sign * np.stack([0.490 + k, zero, zero], axis=1))
    straight2, path = assert_equal(cx, rs, poses, [(1, 1), (1, 0), (0, 1)], reach=0.5, **kw)
    if at_node:
        x = np.abs(xr.thousandths(poses[:, 0]))
        assert (x == 500).any() and (x == 501).any()
        assert np.array_equal(path[x <= 500, 0], 2 * x[x <= 500]) and (path[x > 500] == NONE).all()
        assert np.array_equal(straight2[:, 1], (2600 - x) ** 2) and (straight2[:, 0] == 0).all()


# ---- 2. walls ---------------------------------------------------------------------------------------------------

def sheet(holes=0):
    """A 9 x 9 sheet of carbons 1.5 A apart in the plane y = 0, without its middle (2 holes - 1)^2 atoms."""
    return [("C", (1.5 * (i - 4), 0.0, 1.5 * (j - 4))) for i in range(9) for j in range(9) if holes == 0 or max(abs(i - 4), abs(j - 4)) >= holes]


def shell():
    """150 carbons on a sphere of 4 A about the origin, a golden spiral: every point of the sphere within 0.8 A of a centre."""
    k = np.arange(150)
    z = 1.0 - (2.0 * k + 1.0) / 150.0
    r, g = np.sqrt(1.0 - z * z), np.pi * (3.0 - np.sqrt(5.0))
    return [("C", tuple(np.round(4.0 * np.array([r[i] * np.cos(i * g), r[i] * np.sin(i * g), z[i]]), 3))) for i in k]


WALL_POSE = rigid([(0.0, 4.0, 0.0)])
WALLS = {"wall": 0, "one": 1, "hole": 3}


def wall_case(pkg, tmp_path, what, shift=(0.0, 0.0, 0.0)):
    """An anchor that blocks nothing 4 A below the origin (the receptor's first atom), the sheet `what` (the receptor's
    other atoms), and the ligand, one hydrogen, which WALL_POSE puts 4 A above it -> (complex, restatement, the link)."""
    blockers = sheet(WALLS[what])
    cx, rs = both(pkg, tmp_path, [("H", (0.0, -4.0, 0.0))] + blockers, [("H", (0, 0, 0))], what, shift)
    return cx, rs, [(0, 1 + len(blockers))]


@pytest.mark.parametrize("cell,probe", [(cell, probe) for cell in (0.5, 1.0, 2.0) for probe in (0.0, 1.4)])
@pytest.mark.parametrize("what", ["wall", "one", "hole", "shell"])
def test_walls_holes_and_a_closed_shell(pkg, tmp_path, what, cell, probe):
    """The way round the sheet is 19 to 27 A long, longest on the coarse lattices at the larger probe: max_length 24 at
    h = 500 (a box of 97^3), 28 above."""
    pkg.init(0)
    kw = dict(probe=probe, cell=cell, max_length=24.0 if cell == 0.5 else 28.0)
    h = int(1000 * cell)
    if what == "shell":
        # a closed shell about one anchor: it has doors and no way out
        cx, rs = both(pkg, tmp_path, [("H", (0.0, 0.0, 0.0))] + shell(), [("H", (0, 0, 0))], "shell")
        straight2, path = assert_equal(cx, rs, rigid([(0.0, 10.0, 0.0)]), [(0, 151), (151, 0), (0, 0)], probe=probe, cell=cell, max_length=16.0)
        assert path[0].tolist() == [NONE, NONE, 0] and straight2[0, 0] == 10000 ** 2
        return
    cx, rs, link = wall_case(pkg, tmp_path, what)
    straight2, path = assert_equal(cx, rs, WALL_POSE, link, **kw)
    assert straight2[0, 0] == 8000 ** 2
    if what == "wall":
        assert path[0, 0] != NONE and path[0, 0] > 8000 + 2 * h                      # round the edge
    elif what == "one":
        # one atom left out: its place is 1500 from four carbons of radius 1700, so no node of the plane is free there and
        # the path is the full sheet's
        _, rs_wall, link_wall = wall_case(pkg, tmp_path, "wall")
        assert path[0, 0] == restated(rs_wall, WALL_POSE[0], link_wall, **kw)[1][0] != NONE
    else:
        # the middle 5 x 5 left out: the origin is 4500 from the nearest carbon, free at both probes: straight through
        assert path[0, 0] == 8000


# ---- 3. 1czy ----------------------------------------------------------------------------------------------------

def test_1czy_ranked_poses_with_modes(czy, czy_rs, ranked):
    assert ranked.shape == (3, 27) and czy.pose_len == 27
    links = czy_links(czy_rs)
    assert links[0][0] == links[2][0] == links[3][0]
    straight2, path = assert_equal(czy, czy_rs, ranked, links, max_length=20.0)
    print("1czy, 3 poses x 8 links, 20 A: xlink kernels %.3f ms" % czy.last_kernel_ms())
    # on the restatement alone
    straight = np.sqrt(straight2.astype(np.float64))
    finite = path != NONE
    assert ((finite & (path > straight + 1000)).sum(axis=1) >= 3).all() and (~finite).any() and finite.any()
    # one pose at the full defaults
    _, full = assert_equal(czy, czy_rs, ranked[:1], links)
    print("1czy, 1 pose x 8 links, defaults: xlink kernels %.3f ms" % czy.last_kernel_ms())
    assert (full != NONE).sum() > finite[0].sum()                   # some path is between 20 and 35 A long
    assert np.array_equal(czy.crosslinks(ranked, links, paths=False)["straight2"].astype(np.int64), straight2) and "path" not in czy.crosslinks(ranked, links, paths=False)


# ---- 4. batches -------------------------------------------------------------------------------------------------

def raw_call(lib, cx, poses, links, probe=0.0, cell=1.0, reach=3.0, max_length=12.0, want=(True, True), stride=None, n_links=None):
    """ld_complex_crosslinks on buffers filled with 0xA5 -> (status, straight2, path) (None where not asked for)."""
    poses = np.ascontiguousarray(poses, dtype=np.float64)
    links = None if links is None else np.ascontiguousarray(links, dtype=np.uint32).reshape(-1, 2)
    n, L = len(poses), (len(links) if n_links is None else n_links)
    bufs = [np.full((n, max(L, 1)), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64), np.full((n, max(L, 1)), 0xA5A5A5A5, dtype=np.uint32)]
    bufs = [b if w else None for b, w in zip(bufs, want)]
    ptrs = [None if b is None else b.ctypes.data_as(ctypes.c_void_p) for b in bufs]
    status = lib.ld_complex_crosslinks(cx._h, n, poses.ctypes.data_as(ctypes.c_void_p), poses.shape[1] if stride is None else stride, L,
                                       None if links is None else links.ctypes.data_as(ctypes.c_void_p), ctypes.c_double(probe), ctypes.c_double(cell),
                                       ctypes.c_double(reach), ctypes.c_double(max_length), *ptrs)
    return (status,) + tuple(bufs)


def untouched(bufs):
    return all(b is None or (b.view(np.uint8) == FILL).all() for b in bufs)


def test_batches_slots_strides_link_orders_and_null_outputs(pkg, czy, czy_rs, ranked):
    links = czy_links(czy_rs)
    kw = dict(max_length=12.0)
    straight2, path = wanted(czy_rs, ranked, links, **kw)
    assert (path != NONE).any()
    # the same three poses at 1100 places, rows 30 doubles apart with NaN between them: more jobs than slots
    n = 1100
    source = (np.arange(n) * 7) % 3
    poses = np.full((n, 30), np.nan)
    poses[:, :27] = ranked[source]
    whole = czy.crosslinks(poses, links, **kw)
    print("1100 1czy poses x 8 links, 12 A: xlink kernels %.3f ms" % czy.last_kernel_ms())
    assert np.array_equal(whole["straight2"], straight2[source]) and np.array_equal(whole["path"], path[source])
    pieces = [czy.crosslinks(poses[a:b], links, **kw) for a, b in ((0, 1), (1, 1025), (1025, 1100))]
    for key in ("straight2", "path", "straight"):
        assert np.concatenate([p[key] for p in pieces]).tobytes() == whole[key].tobytes()
    # the links reversed, permuted and duplicated give the permuted words; (a, b) and (b, a) agree
    order = [5, 2, 7, 0, 3, 3, 6, 1, 4, 0]
    mixed = [links[i] for i in order] + [(b, a) for a, b in links]
    got = czy.crosslinks(poses[:9], mixed, **kw)
    for key, want in (("straight2", straight2), ("path", path)):
        assert np.array_equal(got[key][:, :len(order)], want[source[:9]][:, order])
        assert np.array_equal(got[key][:, len(order):], want[source[:9]])
    lib = pkg.load_library()
    for asked in itertools.product((False, True), repeat=2):
        status, s2, p = raw_call(lib, czy, poses[:5], links, want=asked)
        assert status == 0
        assert s2 is None or np.array_equal(s2, whole["straight2"][:5])
        assert p is None or np.array_equal(p, whole["path"][:5])
    empty = czy.crosslinks(np.zeros((0, 27)), links)
    assert empty["straight2"].shape == (0, 8) and empty["path"].shape == (0, 8) and empty["straight"].shape == (0, 8)
    flat = np.ascontiguousarray(links, dtype=np.uint32)
    assert lib.ld_complex_crosslinks(czy._h, 0, None, 27, 8, flat.ctypes.data_as(ctypes.c_void_p), ctypes.c_double(0.0), ctypes.c_double(1.0),
                                     ctypes.c_double(3.0), ctypes.c_double(12.0), None, None) == 0
    bad = poses[:5].copy()
    bad[3, 4] = np.inf
    out = raw_call(lib, czy, bad, links)
    assert out[0] == -1 and untouched(out[1:])


# ---- 5. far from the origin -------------------------------------------------------------------------------------

def test_far_from_the_origin(pkg, tmp_path):
    """The receptor's file 900 000 A out on every axis (its records hold one decimal there, or none), the ligand brought
    there by its pose: differences of 64-bit squares, lattice indices near 10^6."""
    pkg.init(0)
    lib = pkg.load_library()
    k, zero = 0.0005 * np.arange(41), np.zeros(41)
    cx, rs = both(pkg, tmp_path, [("C", (0, 0, 0))], [("C", (0, 0, 0))], "fartwo", FAR)
    poses = rigid(FAR + np.stack([9.990 + k, zero, zero], axis=1))
    links = [(0, 1), (1, 0), (0, 0), (1, 1)]
    straight2, path = assert_equal(cx, rs, poses, links, max_length=12.0)
    x = xr.thousandths(poses[:, 0]) - 900000000
    assert np.array_equal(straight2[:, 0], x * x) and (path[x == 10000, 0] == 10000).all() and (path[x == 10000, 2] == 3464).all()
    assert len(set(path[:, 0].tolist())) > 10
    # a translation that puts an anchor beyond the bound is refused; the receptor's own links still have their straight distance
    for axis, sign in ((0, 1.0), (1, -1.0), (2, 1.0)):
        beyond = poses[:3].copy()
        beyond[1, axis] = sign * 1000000.001
        out = raw_call(lib, cx, beyond, links)
        assert out[0] == -1 and lib.ld_last_error().decode() == "a posed blocker or anchor is beyond +-1.0e6 A" and untouched(out[1:])
        assert raw_call(lib, cx, beyond, [(0, 0)], want=(True, False))[0] == 0
        at = poses[:3].copy()
        at[1, axis] = sign * 1000000.0
        assert raw_call(lib, cx, at, links)[0] == 0
    # the sheet, its hole and the way round it
    kw = dict(max_length=24.0)
    cx, rs, link = wall_case(pkg, tmp_path, "wall", FAR)
    pose = rigid([FAR + np.array([0.0, 4.0, 0.0])])
    straight2, round_the_edge = assert_equal(cx, rs, pose, link, **kw)
    assert straight2[0, 0] == 8000 ** 2 and 10000 < round_the_edge[0, 0] < 24000
    cx, rs, link = wall_case(pkg, tmp_path, "hole", FAR)
    assert assert_equal(cx, rs, pose, link, **kw)[1][0, 0] == 8000


# ---- 6. refusals ------------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched(pkg, czy, czy_rs, ranked, tmp_path):
    lib = pkg.load_library()
    links = czy_links(czy_rs)
    n_atoms = czy.num_atoms(0) + czy.num_atoms(1)

    def refused(poses=ranked, links=links, **kw):
        out = raw_call(lib, czy, poses, links, **kw)
        assert out[0] == -1 and lib.ld_last_error().decode()
        assert untouched(out[1:])

    nan, inf = float("nan"), float("inf")
    for probe in (-0.001, -1.0, 2.001, nan, inf, -inf, 1e300):
        refused(probe=probe)
        with pytest.raises(pkg.LightdockError):
            czy.crosslinks(ranked, links, probe=probe)
    for cell in (0.4994, 0.0, -1.0, 2.0006, nan, inf, -inf, 1e300):
        refused(cell=cell)
    for reach in (0.0004, 0.0, -1.0, 6.0006, nan, inf, -inf, 1e300):
        refused(reach=reach)
    for max_length in (0.9994, 0.0, -1.0, 60.0006, nan, inf, -inf, 1e300):
        refused(max_length=max_length)
    refused(cell=0.5, max_length=40.5)                 # 81 cells
    refused(cell=2.0, max_length=1.999)                # below one cell
    refused(n_links=0)
    refused(links=np.zeros((4097, 2), dtype=np.uint32))
    refused(links=None, n_links=8)
    for bad in (n_atoms, n_atoms + 1, 0xFFFFFFFF):
        for place in ((0, 0), (7, 1)):
            wrong = np.array(links, dtype=np.uint32)
            wrong[place] = bad
            refused(links=wrong)
    for bad in (np.nan, np.inf, -np.inf):
        p = ranked.copy()
        p[1, 5] = bad
        refused(poses=p)
    z = ranked.copy()
    z[2, 3:7] = 0.0
    refused(poses=z)
    refused(poses=ranked[:, :26])                      # stride below the pose length
    over = ranked.copy()
    over[2, 2] = -1.1e6                                # beyond the coordinate bound, found by the kernels
    refused(poses=over)
    refused(poses=over, want=(True, False))
    refused(poses=over, want=(False, True))
    inner = [links[4]]                                 # inside the receptor: its anchors do not move, the ligand's blockers do
    assert raw_call(lib, czy, over, inner, want=(True, False))[0] == 0
    refused(poses=over, links=inner)
    ok = raw_call(lib, czy, ranked, links)
    assert ok[0] == 0 and not untouched(ok[1:])
    # `path` asked for in a complex of which no atom takes part
    rec, lig = pair_of_files(tmp_path, atom(1, "H", "GLY", "A", 1, (0, 0, 0), "H"), atom(1, "BJ", "MMB", "B", 1, (1, 0, 0), "C"), "h")
    cx = pkg.Complex(rec, lig)
    out = raw_call(lib, cx, rigid([(10.0, 0, 0)]), [(0, 1)])
    assert out[0] == -1 and untouched(out[1:])
    status, s2, _ = raw_call(lib, cx, rigid([(10.0, 0, 0)]), [(0, 1)], want=(True, False))
    assert status == 0 and s2.tolist() == [[11000 ** 2]]


# ---- 7. the tool ------------------------------------------------------------------------------------------------

def run_tool(pkg, run, *args, ok=True):
    script = os.path.join(os.path.dirname(pkg.__file__), "xlinks.py")
    r = subprocess.run([sys.executable, script] + list(args), cwd=run, capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr[-2000:]
    return r.stdout, r.stderr


def test_xlinks_tool_on_a_copy_of_the_1czy_run(pkg, czy, czy_rs, tmp_path):
    tool = tool_module("xlinks")
    entries = analyse_module().ranking(range(10), 100, base=CZY)
    run = tmp_path / "run"
    shutil.copytree(CZY, run)
    links = czy_links(czy_rs)
    tables = [tool.atom_table(czy.residues(side), czy.residue_of_atom(side), tool.atom_names(path)) for side, path in ((0, REC), (1, LIG))]
    flat = tables[0] + tables[1]
    limits = [12.0, 25.0, 18.0, 30.0, 9.0, 22.5, 30.0, 15.0]
    text = "# eight links between CA atoms\n"
    for (a, b), limit in zip(links, limits):
        text += "%s %s CA %s %s CA %s\n" % ("R" if a < czy_rs.n_rec else "L", flat[a][0], "R" if b < czy_rs.n_rec else "L", flat[b][0], limit)
    (run / "links.txt").write_text(text)
    assert tool.parse_links(text, tables[0], tables[1])[0] == links

    out, _ = run_tool(pkg, run, "setup.json", "100", "--swarms", "0-9", "--links", "links.txt", "--top", "2")
    print(out.strip())
    lines = open(run / "xlinks" / "rank_xlinks.list").read().splitlines()
    assert "11 models, 8 links measured" in out and lines[0] + "\n" == tool.HEADER and len(lines) == 1 + 11
    rows = [l.split() for l in lines[1:]]
    by_rank = {e[:2]: k for k, e in enumerate(entries)}
    keys = [(-int(r[3].split("/")[0]), float(r[5]), by_rank[(int(r[0]), int(r[1]))]) for r in rows]
    assert keys == sorted(keys) and all(r[3].endswith("/8") and r[4].endswith("/8") for r in rows)        # the order, from the printed columns
    assert sorted((int(r[0]), int(r[1])) for r in rows) == sorted(e[:2] for e in entries)
    assert sorted(os.listdir(run / "xlinks")) == ["links.list", "model_1.pdb", "model_2.pdb", "rank_xlinks.list"]
    listed = open(run / "xlinks" / "links.list").read().splitlines()
    assert listed[0] + "\n" == tool.LINKS_HEADER and len(listed) == 1 + 2 * 8

    # --straight-only against the restatement's straight distances
    out, _ = run_tool(pkg, run, "setup.json", "100", "--swarms", "0-9", "--links", "links.txt", "--straight-only")
    poses = np.array([e[2] for e in entries])
    straight = np.sqrt(np.array([czy_rs.crosslinks(p, links, paths=False)[0] for p in poses], dtype=np.float64)) / 1000.0
    satisfied, by_straight, violation = tool.judge(straight, None, limits, 35.0)
    assert open(run / "xlinks" / "rank_xlinks.list").read() == tool.rank_text(entries, tool.rank_rows(satisfied, violation), satisfied, by_straight, violation, 8)
    assert "straight distances only" in out

    # a line that names no residue fails and cites its line number
    (run / "wrong.txt").write_text(text + "R A.XYZ.9999 CA L %s CA 10\n" % flat[links[0][1]][0])
    _, err = run_tool(pkg, run, "setup.json", "100", "--links", "wrong.txt", ok=False)
    assert "line 10: no residue A.XYZ.9999" in err
