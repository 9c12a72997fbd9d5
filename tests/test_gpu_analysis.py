"""The analysis half of a run on the MI355X (ld_complex_*, lightdock-rust_amd/analyse.py) against the
reference's 1czy products and the numpy restatement of tests/test_analysis_cpu.py."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import bsas_edges
from test_analysis_cpu import CZY, Restated, analyse_module, czy_restated

pytestmark = pytest.mark.gpu

REC = os.path.join(CZY, "lightdock_1czy_protein.pdb")
LIG = os.path.join(CZY, "lightdock_1czy_peptide.pdb")
COORDINATES_TOLERANCE = 1e-9     # A: ld_complex_coordinates against Restated.pose (shared with tests/test_gpu_handle_history.py)


@pytest.fixture(scope="module")
def czy(pkg):
    pkg.init(0)
    return pkg.Complex(REC, LIG, np.load(os.path.join(CZY, "lightdock_rec.nm.npy")), 10,
                       np.load(os.path.join(CZY, "lightdock_lig.nm.npy")), 10)


@pytest.fixture(scope="module")
def czy_rigid(pkg):
    pkg.init(0)
    return pkg.Complex(REC, LIG)


def gso(s):
    return analyse_module().read_gso(os.path.join(CZY, "swarm_%d" % s, "gso_100.out"))


def check_swarm(got, k, want_cluster_of, want_reps):
    n = len(want_reps)
    assert int(got["n_clusters"][k]) == n
    assert np.array_equal(got["cluster_of"][k], want_cluster_of)
    assert list(got["representatives"][k][:n]) == list(want_reps)
    assert np.all(got["representatives"][k][n:] == -1)


def test_analyse_writes_the_reference_products_of_1czy(pkg, tmp_path):
    """analyse.py setup.json 100 --swarms 0-9 --top 10 in a copy of the 1czy run: the ten cluster.repr files,
    rank_by_scoring.list and top_1 / top_2 / top_10 equal what LightDock's tools wrote, byte for byte."""
    run = tmp_path / "run"
    shutil.copytree(CZY, run)
    for s in range(10):
        os.remove(run / ("swarm_%d" % s) / "cluster.repr")
    os.remove(run / "rank_by_scoring.list")
    shutil.rmtree(run / "top")
    script = os.path.join(os.path.dirname(pkg.__file__), "analyse.py")
    r = subprocess.run([sys.executable, script, "setup.json", "100", "--swarms", "0-9", "--top", "10"], cwd=run,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for s in range(10):
        name = os.path.join("swarm_%d" % s, "cluster.repr")
        assert (run / name).read_text() == open(os.path.join(CZY, name)).read(), name
    assert (run / "rank_by_scoring.list").read_text() == open(os.path.join(CZY, "rank_by_scoring.list")).read()
    assert sorted(os.listdir(run / "top")) == sorted("top_%d.pdb" % k for k in range(1, 11))
    for k in (1, 2, 10):
        name = os.path.join("top", "top_%d.pdb" % k)
        assert (run / name).read_bytes() == open(os.path.join(CZY, name), "rb").read(), name


def test_coordinates_agree_with_the_restatement_and_pose_ligand_modes_in_the_ligand_frame(czy):
    rs = czy_restated()
    poses, _ = gso(3)
    got = czy.coordinates(poses[:40])
    assert got.shape == (40, 1281 + 53, 3)
    want = np.stack([rs.pose(p) for p in poses[:40]])
    assert np.max(np.abs(got - want)) < COORDINATES_TOLERANCE
    # a rotated pose with large ligand extents: the ligand-frame convention, not the scoring one
    row = poses[0].copy()
    row[3:7] = [0.3, -0.5, 0.7, 0.4]
    row[17:27] = np.linspace(-3.0, 3.0, 10)
    got = czy.coordinates(row[None])[0]
    assert np.max(np.abs(got - rs.pose(row))) < COORDINATES_TOLERANCE
    assert np.max(np.abs(got[1281:] - rs.pose(row, ligand_frame=False)[1281:])) > 0.1
    assert czy.num_atoms(2) == 175


def test_knife_edge_decisions_equal_the_restatement(czy_rigid):
    """200 poses translate the ligand across RMSD 3.99 - 4.01 A from the representative in small steps."""
    rs = Restated(REC, LIG)
    nb = len(rs.backbone)
    n_lig_bb = sum(1 for i in rs.backbone if i >= 1281)
    d = np.array([1.0, 0.37, -0.52]) / np.linalg.norm([1.0, 0.37, -0.52])
    shift = np.linspace(3.99, 4.01, 199) * np.sqrt(nb / n_lig_bb)   # rmsd = |t| sqrt(n_lig_bb / nb)
    poses = np.zeros((200, 7))
    poses[:, 3] = 1.0
    poses[1:, :3] = shift[:, None] * d
    scoring = 100.0 - np.arange(200.0)
    got = czy_rigid.cluster(poses[None], scoring[None], 4.0)
    want_of, want_reps, knife = rs.bsas(poses, scoring, 4.0)
    print("knife-edge comparisons: %d" % knife)
    # the exact integer rule on the thousandths the tool re-reads (tests/bsas_edges.py): n = 175 admits no tie (16 does not
    # divide it), so nothing is excused
    T = np.array([np.rint(rs.backbone_printed(p) * 1000.0).astype(np.int64).ravel() for p in poses])
    exact_of, exact_reps, ties = bsas_edges.bsas(T, nb, scoring, 4.0)
    assert ties == 0 and nb % 16 != 0
    check_swarm(got, 0, exact_of, exact_reps)
    if knife == 0:
        check_swarm(got, 0, want_of, want_reps)
    assert 1 < len(exact_reps)   # the steps do cross the cutoff


def test_equal_scores_cluster_in_glowworm_order(czy_rigid):
    near = np.array([0, 0, 0, 1, 0, 0, 0.0])
    far = np.array([40, 0, 0, 1, 0, 0, 0.0])
    poses = np.stack([far, near, far, near, near, far])
    got = czy_rigid.cluster(poses[None], np.zeros((1, 6)), 4.0)
    check_swarm(got, 0, [0, 1, 0, 1, 1, 0], [0, 1])
    scoring = np.array([[1.0, 1.0, 1.0, 1.0, 7.0, 1.0]])   # glowworm 4 first, then index order
    got = czy_rigid.cluster(poses[None], scoring, 4.0)
    check_swarm(got, 0, [1, 0, 1, 0, 0, 1], [4, 0])


def random_poses(rng, n, cols):
    p = np.zeros((n, cols))
    p[:, :3] = rng.uniform(-20, 20, (n, 3))
    q = rng.normal(size=(n, 4))
    p[:, 3:7] = q / np.linalg.norm(q, axis=1)[:, None]
    p[:, 7:] = rng.normal(0, 0.5, (n, cols - 7))
    return p


def test_extremes(czy):
    rng = np.random.default_rng(7)
    one = czy.cluster(random_poses(rng, 1, 27)[None], np.array([[2.5]]), 4.0)
    check_swarm(one, 0, [0], [0])
    poses = random_poses(rng, 4096, 27)[None]
    scoring = rng.normal(size=(1, 4096))
    order = sorted(range(4096), key=lambda i: scoring[0, i], reverse=True)
    every = czy.cluster(poses, scoring, 0.0)                  # every glowworm its own cluster: 4096 rounds
    rank = np.empty(4096, dtype=np.int64)
    rank[order] = np.arange(4096)
    check_swarm(every, 0, rank, order)
    single = czy.cluster(poses, scoring, 1e9)
    check_swarm(single, 0, np.zeros(4096), [order[0]])


def test_rigid_1ppe_and_dna_1azp_against_the_restatement(pkg):
    from conftest import GOLDEN
    rng = np.random.default_rng(11)
    pkg.init(0)
    d = os.path.join(GOLDEN, "1ppe")
    rec, lig = os.path.join(d, "lightdock_1ppe_e.pdb"), os.path.join(d, "lightdock_1ppe_i.pdb")
    cx = pkg.Complex(rec, lig)
    assert cx.pose_len == 7
    poses = np.loadtxt(os.path.join(d, "initial_positions_0.dat"))[:120, :7]
    poses[:, :3] += rng.normal(0, 1.5, (120, 3))
    scoring = rng.normal(size=120)
    got = cx.cluster(poses[None], scoring[None], 4.0)
    want_of, want_reps, knife = Restated(rec, lig).bsas(poses, scoring, 4.0)
    assert knife == 0
    check_swarm(got, 0, want_of, want_reps)
    d = os.path.join(GOLDEN, "1azp")
    rec, lig = os.path.join(d, "lightdock_protein.pdb"), os.path.join(d, "lightdock_dna.pdb")
    rnm, lnm = np.load(os.path.join(d, "rec_nm.npy")), np.load(os.path.join(d, "lig_nm.npy"))
    cx = pkg.Complex(rec, lig, rnm, 10, lnm, 10)
    rs = Restated(rec, lig, rnm, lnm)
    n_p = sum(1 for line in open(lig) if line.startswith("ATOM") and line[12:16].strip() == "P")
    assert n_p > 0 and cx.num_atoms(2) == len(rs.backbone)
    poses = np.loadtxt(os.path.join(d, "initial_positions_0.dat"))[:80]
    poses[:, :3] += rng.normal(0, 1.0, (80, 3))
    scoring = rng.normal(size=80)
    got = cx.cluster(poses[None], scoring[None], 4.0)
    want_of, want_reps, knife = rs.bsas(poses, scoring, 4.0)
    assert knife == 0
    check_swarm(got, 0, want_of, want_reps)
    assert np.max(np.abs(cx.coordinates(poses[:5]) - np.stack([rs.pose(p) for p in poses[:5]]))) < COORDINATES_TOLERANCE


def perturbed_czy(rng, n_swarms):
    base = np.stack([gso(s)[0] for s in range(10)])
    poses = base[np.arange(n_swarms) % 10].copy()
    poses[:, :, :3] += rng.normal(0, 1.0, poses[:, :, :3].shape)
    q = poses[:, :, 3:7] + rng.normal(0, 0.05, poses[:, :, 3:7].shape)
    poses[:, :, 3:7] = q / np.linalg.norm(q, axis=2)[:, :, None]
    poses[:, :, 7:] += rng.normal(0, 0.1, poses[:, :, 7:].shape)
    return poses, rng.normal(10.0, 3.0, poses.shape[:2])


def test_1024_swarms_in_one_call(czy):
    rng = np.random.default_rng(5)
    poses, scoring = perturbed_czy(rng, 1024)
    got = czy.cluster(poses, scoring, 4.0)
    for k in range(1024):
        n = int(got["n_clusters"][k])
        assert np.bincount(got["cluster_of"][k], minlength=n).sum() == 200 and got["cluster_of"][k].max() == n - 1
    rs = czy_restated()
    for k in (0, 1, 9, 137, 500, 511, 777, 1023):
        want_of, want_reps, knife = rs.bsas(poses[k], scoring[k], 4.0)
        assert knife == 0
        check_swarm(got, k, want_of, want_reps)


def test_errors_return_invalid_and_write_nothing(pkg, czy, tmp_path):
    lib = pkg.load_library()
    good = gso(0)[0][:4]
    out = tmp_path / "x.pdb"

    def invalid(call):
        with pytest.raises(pkg.LightdockError) as e:
            call()
        assert e.value.status == -1 and lib.ld_last_error().decode()
        assert not out.exists()

    for bad in (np.nan, np.inf):
        p = good.copy()
        p[2, 5] = bad
        invalid(lambda: czy.cluster(p[None], np.ones((1, 4))))
        invalid(lambda: czy.coordinates(p))
        invalid(lambda: czy.write_pdb(p[2], str(out)))
        invalid(lambda: czy.cluster(good[None], np.array([[1.0, bad, 2.0, 3.0]])))
    z = good.copy()
    z[1, 3:7] = 0.0
    invalid(lambda: czy.cluster(z[None], np.ones((1, 4))))
    invalid(lambda: czy.write_pdb(z[1], str(out)))
    invalid(lambda: czy.cluster(np.zeros((1, 0, 27)), np.zeros((1, 0))))
    invalid(lambda: czy.cluster(np.tile(good, (1025, 1))[None], np.ones((1, 4100))))
    rnm = np.load(os.path.join(CZY, "lightdock_rec.nm.npy"))
    invalid(lambda: pkg.Complex(REC, LIG, rnm.ravel()[:-3], 10))
    invalid(lambda: pkg.Complex(REC, LIG, rnm, 9))
    noca = tmp_path / "noca.pdb"
    noca.write_text("".join(l for l in open(LIG) if l[12:16].strip() not in ("CA", "P")))
    cx = pkg.Complex(str(noca), str(noca))
    invalid(lambda: cx.cluster(np.array([[[0, 0, 0, 1, 0, 0, 0.0]]]), np.ones((1, 1))))
    czy.write_pdb(good[0], str(out))          # and the good pose does write
    assert out.exists()
