"""The density fit on the MI355X (ld_complex_density_fit, ld_complex_simulate_density, lightdock-rust_amd/emfit.py; DESIGN
§5 K3i).  Voxels and sums are compared word for word with the int64 / Python-integer restatement of
tests/emfit_reference.py.

The knife edges: d^2 = (t << s) - 1 is 7 modulo 8 for every shift the rule gives (s >= 9), and no such number is a sum of
three squares, so no atom can stand there; the edges are read at the nearest d^2 that exist on either side, (t << s) - 2 or
lower and t << s or higher, found by search and asserted to straddle the edge."""
import ctypes
import hashlib
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import emfit_reference as er
from test_analysis_cpu import CZY, analyse_module, tool_module
from test_gpu_contacts import REC, LIG, perturbed_czy
from test_gpu_sasa import atom, pair_of_files

pytestmark = pytest.mark.gpu

FILL = 0xA5
KEYS = ("s", "ss", "se", "inside_sum", "outside")
ZN = atom(1, "ZN", "ZN", "A", 1, (0.0, 0.0, 0.0), "ZN", True)


def rigid(t):
    t = np.asarray(t, dtype=np.float64).reshape(-1, 3)
    poses = np.zeros((len(t), 7))
    poses[:, :3] = t
    poses[:, 3] = 1.0
    return poses


def three_squares(lo, hi, step):
    """The first m in lo, lo + step, .. (towards hi, exclusive) that is a sum of three squares -> (m, (x, y, z))."""
    for m in range(lo, hi, step):
        for x in range(math.isqrt(m), max(math.isqrt(m) - 40, -1), -1):
            rem = m - x * x
            ys = np.arange(0, math.isqrt(rem) + 1, dtype=np.int64)
            z2 = rem - ys * ys
            z = np.floor(np.sqrt(z2.astype(np.float64))).astype(np.int64)
            z += ((z + 1) * (z + 1) <= z2)
            z -= (z * z > z2)
            hit = np.flatnonzero(z * z == z2)
            if len(hit):
                return m, (x, int(ys[hit[0]]), int(z[hit[0]]))
    raise AssertionError("no sum of three squares in range")


def fit_and_voxels(cx, rs, poses, dens, E, origin, step, sigma):
    """density_fit and simulate_density against the restatement, word for word -> the sums."""
    got = cx.density_fit(poses, dens, sigma)
    grids = cx.simulate_density(poses, dens, sigma)
    want = [rs.fit(p, E, origin, step, sigma) for p in poses]
    assert grids.dtype == np.uint32 and grids.shape == (len(poses),) + E.shape
    for i, (w, g) in enumerate(want):
        assert np.array_equal(grids[i], g), i
    assert er.same_words(got, [w for w, _ in want]), (got, [w for w, _ in want])
    # the sums are the sums of simulate_density's own voxels
    for i in range(len(poses)):
        own = er.sums_of(grids[i], E)
        assert all(int(got[k][i]) == own[k] for k in KEYS[:4])
    return got


@pytest.fixture(scope="module")
def one_carbon(pkg, tmp_path_factory):
    pkg.init(0)
    rec, lig = pair_of_files(tmp_path_factory.mktemp("zc"), ZN, atom(1, "C", "GLY", "B", 1, (0, 0, 0), "C"))
    return pkg.Complex(rec, lig), er.EmfitRestated(rec, lig)


@pytest.fixture(scope="module")
def czy(pkg):
    pkg.init(0)
    return pkg.Complex(REC, LIG, np.load(os.path.join(CZY, "lightdock_rec.nm.npy")), 10,
                       np.load(os.path.join(CZY, "lightdock_lig.nm.npy")), 10)


CZY_SHAPE, CZY_STEP, CZY_SIGMA = (26, 22, 24), (3000, 3000, 3000), 2250     # 24 x 22 x 26 voxels of 3 A at 10 A resolution


@pytest.fixture(scope="module")
def ranked(pkg):
    """Five of the eleven ranked models of the 1czy run, a synthetic map around them and their restated fits: made once."""
    pkg.init(0)
    entries = analyse_module().ranking(range(10), 100, base=CZY)
    poses = np.array([e[2] for e in entries])[[0, 2, 5, 8, 10]]
    rs = er.czy_emfit()
    t = rs.thousandths(poses[0])
    origin = tuple(int(v) - 4000 for v in t.min(axis=0))
    rng = np.random.default_rng(3)
    rho = rng.normal(0.2, 1.0, CZY_SHAPE).astype(np.float32)
    dens = pkg.Density(rho, origin, CZY_STEP)
    E = dens.voxels().astype(np.int64)
    want = [rs.fit(p, E, origin, CZY_STEP, CZY_SIGMA) for p in poses]
    return poses, dens, E, origin, want


# ---- 1. knife edges ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sigma,h", [(300, 1000), (2250, 1000), (15000, 20000)])
def test_knife_edges_of_the_table(pkg, one_carbon, tmp_path, sigma, h):
    cx, rs = one_carbon
    table, shift = pkg.density_kernel(sigma)
    T = len(table)
    dens = pkg.Density(np.ones((1, 1, 1), dtype=np.float32), (0, 0, 0), (h, h, h))
    places, want = [], []
    for t in (1, 2, 7, T // 3, T // 2, T - 1, T):
        below, at = three_squares((t << shift) - 2, ((t - 1) << shift) - 1, -1), three_squares(t << shift, (t + 1) << shift, 1)
        assert below[0] >> shift == t - 1 and (at[0] >> shift == t) and (t << shift) - below[0] <= 8 and at[0] - (t << shift) <= 8
        places += [below[1], at[1]]
        want += [6 * int(table[t - 1]), 6 * int(table[t]) if t < T else 0]
    # permuted and mirrored: every axis carries the large difference once
    places += [(-p[1], p[2], -p[0]) for p in places] + [(p[2], -p[0], p[1]) for p in places]
    want = want * 3
    poses = rigid(np.array(places) / 1000.0)
    got = cx.simulate_density(poses, dens, sigma)
    assert got.reshape(-1).tolist() == want
    assert want[-1] == 0 and want[-2] == 6 * int(table[T - 1]) and want[-2] in (0, 6)     # (T << s) - 2 adds K[T - 1]; T << s nothing
    if sigma == 15000:
        assert (T << shift) > 2 ** 31 and max(max(abs(v) for v in p) for p in places) > 46341   # a square alone passes 2^31
        # and d^2 beyond 2^32 and 2^33, on one axis and on three: nothing, no wrap
        far = rigid([(65.537, 0, 0), (0, -92.7, 0), (60.0, 60.0, 60.0), (0, 0, 2000.0), (-9.0e5, 9.0e5, 9.0e5)])
        assert cx.simulate_density(far, dens, sigma).reshape(-1).tolist() == [0] * 5
    fit = cx.density_fit(poses, dens, sigma)
    assert fit["s"].tolist() == want and fit["ss"].tolist() == [w * w for w in want] and fit["se"].tolist() == [w * 32767 for w in want]
    assert fit["inside_sum"].tolist() == want
    outside = [int(any(2 * v < -h or 2 * v >= h for v in p)) for p in places]
    assert fit["outside"].tolist() == outside and 0 in outside and 1 in outside
    # the same edges on the rigid-receptor path: a hydrogen far from the map joins the zinc, so the receptor is deposited once
    rec, lig = pair_of_files(tmp_path, ZN + atom(2, "H", "GLY", "A", 2, (900.0, 900.0, 900.0), "H"), atom(1, "C", "GLY", "B", 1, (0, 0, 0), "C"))
    based = pkg.Complex(rec, lig)
    assert np.array_equal(based.simulate_density(poses, dens, sigma), got)
    fit2 = based.density_fit(poses, dens, sigma)
    assert all(np.array_equal(fit2[k], fit[k]) for k in KEYS[:4]) and fit2["outside"].tolist() == [o + 1 for o in outside]
    grids = [rs.grid(p, (1, 1, 1), (0, 0, 0), (h, h, h), sigma) for p in poses[:6]]
    assert [int(g[0, 0, 0]) for g in grids] == want[:6]


# ---- 2. clipping and `outside` ----------------------------------------------------------------------------------

def test_supports_that_leave_the_map_and_the_half_cell_edges(pkg, one_carbon):
    cx, rs = one_carbon
    shape, origin, step, sigma = (5, 3, 4), (-2000, 1000, 500), (1500, 1000, 1250), 900        # reach 3.178 A
    rng = np.random.default_rng(17)
    dens = pkg.Density(rng.uniform(-0.5, 1.0, shape).astype(np.float32), origin, step)
    E = dens.voxels().astype(np.int64)
    last = [origin[k] + (shape[2 - k] - 1) * step[k] for k in range(3)]
    mid = [(origin[k] + last[k]) // 2 for k in range(3)]
    places = []
    for k in range(3):                                     # beyond each of the six faces, the support still reaching in
        for v in (origin[k] - 2000, last[k] + 2000):
            p = list(mid)
            p[k] = v
            places.append(p)
    places.append([origin[0] - 3100, origin[1] - 300, mid[2]])            # a corner: only a few voxels within reach
    places.append([origin[0] - 3179, mid[1], mid[2]])                     # wholly outside: 3179 > reach
    places.append([last[0] + 9000, last[1] + 9000, last[2] + 9000])
    for k in range(3):                                     # the half-cell edges: -h/2 - 1, -h/2, +h/2 - 1, +h/2 about the end centres
        h = step[k]
        for v in (origin[k] - h // 2 - 1, origin[k] - h // 2, last[k] + h // 2 - 1, last[k] + h // 2):
            p = list(mid)
            p[k] = v
            places.append(p)
    poses = rigid(np.array(places) / 1000.0)
    got = fit_and_voxels(cx, rs, poses, dens, E, origin, step, sigma)
    assert got["outside"][:6].tolist() == [1] * 6 and (got["s"][:6] > 0).all()
    assert got["outside"][7:9].tolist() == [1, 1] and all(got[k][7:9].tolist() == [0, 0] for k in KEYS[:4])
    assert got["outside"][9:].tolist() == [1, 0, 0, 1] * 3


# ---- 3. shapes --------------------------------------------------------------------------------------------------

ELEMENTS = ("C", "N", "O", "S", "H", "P")
MAPS = (((33, 15, 1), (1500, 2000, 2500)), ((1, 17, 16), (2500, 1500, 2000)), ((17, 16, 33), (2000, 2500, 1500)),
        ((16, 33, 15), (1500, 1500, 1500)), ((15, 1, 17), (2200, 1700, 1900)))        # (nz, ny, nx), (hx, hy, hz)


def random_file(rng, n, chain, first=0):
    xyz = rng.uniform(-20.0, 20.0, (n, 3))
    return "".join(atom(i + 1, ELEMENTS[(first + i) % 6], "UNK", chain, i + 1, xyz[i], ELEMENTS[(first + i) % 6]) for i in range(n))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("heavy", ["receptor", "ligand"])
def test_sizes_around_the_wave_the_tile_and_the_brick(pkg, tmp_path, n, heavy):
    """n atoms take part, random in a box of 40 A, all but one (or all, at n = 1) on the heavy side; a zinc fills a side
    that would be empty.  Two maps of the five, so that every size of an axis (1, 15, 16, 17, 33) meets every n."""
    pkg.init(0)
    rng = np.random.default_rng(2000 + n)
    single = random_file(rng, 1, "A")
    rest = random_file(rng, n - 1, "B", 1) if n > 1 else ZN
    rec, lig = pair_of_files(tmp_path, *((rest, single) if heavy == "receptor" else (single, rest)))
    cx, rs = pkg.Complex(rec, lig), er.EmfitRestated(rec, lig)
    assert rs.n_part == n
    poses = rigid([(0, 0, 0), (3.3, -2.2, 1.1), (-14.0, 20.5, 2.5)])
    poses[1, 3:7] = [0.1, -0.7, 0.3, 0.64]                 # not normalised: the posing divides by the norm
    poses[2, 3:7] = [0.0, 0.0, 1.0, 0.0]
    at = [1, 63, 64, 65, 257].index(n)
    for shape, step in (MAPS[at], MAPS[(at + 2) % 5]):
        origin = (-18000 - 7 * n, -12000 + n, -21000)
        dens = pkg.Density(rng.uniform(-0.3, 1.0, shape).astype(np.float32), origin, step)
        fit_and_voxels(cx, rs, poses, dens, dens.voxels().astype(np.int64), origin, step, 900)


def test_atoms_on_brick_boundaries(pkg, tmp_path):
    """Atoms on the centre of voxel 15, of voxel 16 (the next brick's first) and half way between them, on every axis."""
    pkg.init(0)
    shape, origin, step = (33, 17, 18), (-9000, -4000, -20000), (1000, 1200, 1100)
    spots = [(origin[0] + i * step[0], origin[1] + j * step[1], origin[2] + k * step[2]) for i, j, k in ((15, 15, 15), (16, 16, 16), (16, 3, 31), (2, 16, 32))]
    spots += [(origin[0] + 15 * step[0] + step[0] // 2, origin[1] + 15 * step[1] + step[1] // 2, origin[2] + 15 * step[2] + step[2] // 2)]
    text = "".join(atom(i + 1, "O", "HOH", "B", i + 1, np.array(s) / 1000.0, "O", True) for i, s in enumerate(spots))
    rec, lig = pair_of_files(tmp_path, atom(1, "SG", "CYS", "A", 1, np.array(spots[1]) / 1000.0, "S"), text)
    cx, rs = pkg.Complex(rec, lig), er.EmfitRestated(rec, lig)
    dens = pkg.Density(np.random.default_rng(4).uniform(0, 1, shape).astype(np.float32), origin, step)
    got = fit_and_voxels(cx, rs, rigid([(0, 0, 0), (0.0005, -0.0005, -1.1)]), dens, dens.voxels().astype(np.int64), origin, step, 600)
    assert got["outside"].tolist() == [0, 0]


# ---- 4. 1czy with its modes -------------------------------------------------------------------------------------

def test_1czy_ranked_models(czy, ranked):
    poses, dens, E, origin, want = ranked
    got = czy.density_fit(poses, dens, CZY_SIGMA)
    assert er.same_words(got, [w for w, _ in want])
    grids = czy.simulate_density(poses, dens, CZY_SIGMA)
    for i, (_, g) in enumerate(want):
        assert np.array_equal(grids[i], g)
    assert (got["s"] > 0).all() and len(set(got["se"].tolist())) == 5


def test_batches_of_1_7_and_300_give_identical_rows(czy, ranked):
    poses, dens, E, origin, want = ranked
    rows = [w for w, _ in want]
    filler = perturbed_czy(np.random.default_rng(8), 2).reshape(-1, 27)[:300]
    for i, p in enumerate(poses):
        assert er.same_words(czy.density_fit(p[None, :], dens, CZY_SIGMA), rows[i:i + 1])
    seven = filler[:7].copy()
    seven[[1, 2, 4, 5, 6]] = poses
    got = czy.density_fit(seven, dens, CZY_SIGMA)
    assert er.same_words({k: got[k][[1, 2, 4, 5, 6]] for k in KEYS}, rows)
    at = [0, 17, 150, 298, 299]
    big = filler.copy()
    big[at] = poses
    got = czy.density_fit(big, dens, CZY_SIGMA)
    assert er.same_words({k: got[k][at] for k in KEYS}, rows)
    again = czy.density_fit(filler[[1, 2, 3]], dens, CZY_SIGMA)
    assert all(np.array_equal(again[k], got[k][[1, 2, 3]]) for k in KEYS)


def test_more_poses_than_a_chunk_holds(czy, ranked):
    poses, dens, E, origin, want = ranked
    seven = np.concatenate([poses, poses[:2]])
    rows = [w for w, _ in want] + [w for w, _ in want[:2]]
    for chunk in (1, 2, 3, 7, 100):
        assert er.same_words(czy.density_fit(seven, dens, CZY_SIGMA, chunk=chunk), rows)
    grids = czy.simulate_density(seven, dens, CZY_SIGMA, chunk=3)
    assert all(np.array_equal(grids[i], want[i % 5][1]) for i in range(7))


def test_a_receptor_without_modes_equals_zero_amplitude_modes(pkg, ranked):
    """Without receptor modes the receptor is deposited once a call and a pose visits only the bricks its ligand reaches;
    with modes of amplitude zero every pose deposits all its atoms.  Also with the ligand partly and wholly outside the map."""
    poses, dens, E, origin, _ = ranked
    rec_nm, lig_nm = np.load(os.path.join(CZY, "lightdock_rec.nm.npy")), np.load(os.path.join(CZY, "lightdock_lig.nm.npy"))
    still = np.concatenate([poses, poses[:3]])
    still[:, 7:17] = 0.0
    still[5, :3] += (30.0, 0.0, 0.0)                       # towards a face
    still[6, :3] = (origin[0] / 1000.0 - 3.0, origin[1] / 1000.0 + 20.0, origin[2] / 1000.0 + 20.0)   # across a face
    still[7, :3] = (500.0, -500.0, 500.0)                  # wholly outside
    no_modes = pkg.Complex(REC, LIG, None, 0, lig_nm, 10)
    with_modes = pkg.Complex(REC, LIG, rec_nm, 10, lig_nm, 10)
    short = np.concatenate([still[:, :7], still[:, 17:]], axis=1)
    a, b = no_modes.density_fit(short, dens, CZY_SIGMA), with_modes.density_fit(still, dens, CZY_SIGMA)
    assert all(np.array_equal(a[k], b[k]) for k in KEYS)
    assert a["outside"][7] > a["outside"][0]              # every ligand atom is outside; the restatement below pins the count
    ga, gb = no_modes.simulate_density(short, dens, CZY_SIGMA), with_modes.simulate_density(still, dens, CZY_SIGMA)
    assert np.array_equal(ga, gb)
    rs = er.czy_emfit()
    want = [rs.fit(p, E, origin, CZY_STEP, CZY_SIGMA) for p in still[5:]]
    assert er.same_words({k: a[k][5:] for k in KEYS}, [w for w, _ in want]) and all(np.array_equal(ga[5 + i], want[i][1]) for i in range(3))
    for chunk in (1, 3):
        c = no_modes.density_fit(short, dens, CZY_SIGMA, chunk=chunk)
        assert all(np.array_equal(a[k], c[k]) for k in KEYS)


# ---- 5. overflow and refusals -----------------------------------------------------------------------------------

def raw_fit(lib, cx, dens, poses, sigma=CZY_SIGMA, stride=None, simulate=False, voxels=1):
    """ld_complex_density_fit (or _simulate_density) on a buffer filled with 0xA5 -> (status, untouched)."""
    poses = np.ascontiguousarray(poses, dtype=np.float64)
    n = len(poses)
    buf = np.full(n * (4 * voxels if simulate else 40), FILL, dtype=np.uint8)
    call = lib.ld_complex_simulate_density if simulate else lib.ld_complex_density_fit
    status = call(cx._h, dens._h if dens is not None else None, n, poses.ctypes.data_as(ctypes.c_void_p), poses.shape[1] if stride is None else stride, sigma,
                  buf.ctypes.data_as(ctypes.c_void_p))
    return status, bool((buf == FILL).all())


def test_a_voxel_at_2_to_the_24_is_refused_and_one_below_is_not(pkg, tmp_path):
    """4113 sulfurs on one voxel's centre add 4113 x 16 x 255 = 16781040 >= 2^24; 4112 add 16776960."""
    pkg.init(0)
    lib = pkg.load_library()
    dens = pkg.Density(np.ones((2, 2, 2), dtype=np.float32), (0, 0, 0), (1000, 1000, 1000))
    poses = rigid([(0, 0, 0), (9.0, 9.0, 9.0)])
    for count, refused in ((4112, False), (4113, True)):
        pile = "".join(atom(i + 1, "SG", "CYS", "B", 1 + i % 9000, (0, 0, 0), "S") for i in range(count))
        for tag, (rec, lig) in (("l", (ZN, pile)), ("r", (pile, atom(1, "ZN", "ZN", "B", 1, (0, 0, 0), "ZN", True)))):
            cx = pkg.Complex(*pair_of_files(tmp_path, rec, lig, "%s%d" % (tag, count)))
            first = poses[:1] if tag == "l" else poses
            assert raw_fit(lib, cx, dens, first, 300) == ((-1, True) if refused else (0, False))
            assert raw_fit(lib, cx, dens, first, 300, simulate=True, voxels=8) == ((-1, True) if refused else (0, False))
            if refused:
                assert "2^24" in lib.ld_last_error().decode()
                if tag == "l":                             # the pile away from the map: the pose is fine again, and alone
                    assert raw_fit(lib, cx, dens, poses[1:], 300) == (0, False) and raw_fit(lib, cx, dens, poses, 300) == (-1, True)
            else:
                assert int(cx.simulate_density(first, dens, 300)[0, 0, 0, 0]) == count * 16 * 255


def test_refusals_by_status_with_the_outputs_untouched(pkg, czy, ranked, tmp_path):
    poses, dens, E, origin, _ = ranked
    poses = poses[:3]
    lib = pkg.load_library()
    N = int(np.prod(CZY_SHAPE))
    assert raw_fit(lib, czy, dens, poses) == (0, False) and raw_fit(lib, czy, dens, poses, simulate=True, voxels=N) == (0, False)
    for kw in (dict(sigma=299), dict(sigma=15001), dict(sigma=0), dict(stride=26), dict(stride=0)):
        assert raw_fit(lib, czy, dens, poses, **kw) == (-1, True), kw
        assert raw_fit(lib, czy, dens, poses, simulate=True, voxels=N, **kw) == (-1, True), kw
        assert lib.ld_last_error().decode()
    # a support wider than 16 voxels: isqrt(T << s) = 48.7 A at sigma 13.8 A against 16 x 3 A; 13.5 A fits
    assert raw_fit(lib, czy, dens, poses, sigma=13800) == (-1, True) and "16 voxels" in lib.ld_last_error().decode()
    assert raw_fit(lib, czy, dens, poses, sigma=13500)[0] == 0
    for bad in (np.nan, np.inf, -np.inf):
        p = poses.copy()
        p[1, 12] = bad
        assert raw_fit(lib, czy, dens, p) == (-1, True) and raw_fit(lib, czy, dens, p, simulate=True, voxels=N) == (-1, True)
    z = poses.copy()
    z[2, 3:7] = 0.0
    assert raw_fit(lib, czy, dens, z) == (-1, True)
    far = poses.copy()
    far[0, 1] = 1.1e6                                       # beyond the coordinate bound
    assert raw_fit(lib, czy, dens, far) == (-1, True)
    assert raw_fit(lib, czy, None, poses) == (-1, True)
    assert lib.ld_complex_density_fit(czy._h, dens._h, 3, poses.ctypes.data_as(ctypes.c_void_p), 27, CZY_SIGMA, None) == -1
    assert lib.ld_complex_density_fit(czy._h, dens._h, 0, None, 27, CZY_SIGMA, None) == 0
    assert lib.ld_complex_simulate_density(czy._h, dens._h, 0, None, 27, CZY_SIGMA, None) == 0
    # more than 256 MiB of voxels: 4889 poses x 13728 voxels x 4 B
    many = np.repeat(poses[:1], 4889, axis=0)
    assert lib.ld_complex_simulate_density(czy._h, dens._h, len(many), many.ctypes.data_as(ctypes.c_void_p), 27, CZY_SIGMA, None) == -1
    with pytest.raises(pkg.LightdockError):
        czy.simulate_density(many, dens, CZY_SIGMA)
    # a complex in which no atom takes part
    rec, lig = pair_of_files(tmp_path, ZN, atom(1, "ZN", "ZN", "B", 1, (0, 0, 0), "ZN", True) + atom(2, "BJ", "MMB", "B", 2, (1, 0, 0), "C", True))
    zn = pkg.Complex(rec, lig)
    assert raw_fit(lib, zn, dens, rigid([(1, 0, 0), (2, 0, 0)])) == (-1, True)
    with pytest.raises(pkg.LightdockError):
        zn.density_fit(rigid([(1, 0, 0)]), dens, CZY_SIGMA)


# ---- 6. emfit.py end to end -------------------------------------------------------------------------------------

def snapshot(root):
    out = {}
    for d, _, files in os.walk(root):
        if os.path.basename(d) == "emfit" and os.path.dirname(d) == str(root):
            continue
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = hashlib.sha256(open(p, "rb").read()).hexdigest()
    return out


def run_emfit(pkg, run, *args):
    script = os.path.join(os.path.dirname(pkg.__file__), "emfit.py")
    r = subprocess.run([sys.executable, script] + list(args), cwd=run, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout, open(os.path.join(run, "emfit", "rank_emfit.list")).read()


def test_emfit_tool_on_a_copy_of_the_1czy_run(pkg, tmp_path):
    """A first run on a blank map of the complex's extent writes the simulated map of every candidate; the chosen one's
    becomes the "experimental" map of a second run, which must rank that candidate first."""
    tool = tool_module("emfit")
    entries = analyse_module().ranking(range(10), 100, base=CZY)
    chosen = 4
    run, maps = tmp_path / "run", tmp_path / "maps"
    shutil.copytree(CZY, run)
    os.makedirs(maps)
    t = er.czy_emfit().thousandths(entries[0][2])
    origin = tuple(int(v) // 1000 * 1000 - 9000 for v in t.min(axis=0))
    shape = tuple(int(math.ceil((int(t[:, k].max()) - origin[k]) / 3000.0)) + 4 for k in (2, 1, 0))
    tool.write_mrc(str(maps / "blank.mrc"), np.ones(shape, dtype=np.float32), origin, (3000, 3000, 3000))
    before = snapshot(run)
    out, text = run_emfit(pkg, run, "setup.json", "100", "--swarms", "0-9", "--map", str(maps / "blank.mrc"), "--resolution", "10", "--write-map", "11")
    assert "11 models fitted" in out
    first = [l.split() for l in text.splitlines()[1:]]
    k = [(int(r[0]), int(r[1])) for r in first].index((entries[chosen][0], entries[chosen][1])) + 1
    shutil.copy(run / "emfit" / ("model_%d.mrc" % k), maps / "exp.mrc")
    shutil.rmtree(run / "emfit")
    out, text = run_emfit(pkg, run, "setup.json", "100", "--swarms", "0-9", "--map", str(maps / "exp.mrc"), "--resolution", "10", "--top", "2", "--write-map", "1")
    lines = text.splitlines()
    assert lines[0].split() == ["Swarm", "Glowworm", "Scoring", "cc", "ccm", "inside", "outside"] and len(lines) == 12
    rows = [l.split() for l in lines[1:]]
    assert (int(rows[0][0]), int(rows[0][1])) == (entries[chosen][0], entries[chosen][1])
    cc, ccm = [float(r[3]) for r in rows], [float(r[4]) for r in rows]
    assert ccm == sorted(ccm, reverse=True) and ccm[0] > ccm[1] and ccm[0] > 0.9999
    assert all(-1.0 <= v <= 1.0 for v in cc + ccm) and all(0.0 <= float(r[5]) <= 1.0 for r in rows)
    assert sorted((int(r[0]), int(r[1])) for r in rows) == sorted((e[0], e[1]) for e in entries)
    assert sorted(os.listdir(run / "emfit")) == ["model_1.mrc", "model_1.pdb", "model_2.pdb", "rank_emfit.list"]
    # the map written for the first row is the experimental map again: the same voxels
    again, exp = tool.read_mrc(str(run / "emfit" / "model_1.mrc")), tool.read_mrc(str(maps / "exp.mrc"))
    assert np.array_equal(again[0], exp[0]) and again[1:3] == exp[1:3] == (origin, (3000, 3000, 3000))
    assert snapshot(run) == before                           # nothing else in the run directory changes
