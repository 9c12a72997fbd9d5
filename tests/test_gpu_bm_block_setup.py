"""GPU tests of dfire_bm_pairs' block set-up (run with -m gpu on an MI355X).

At every block of a job a wave forms the block's item list -- lane-major: a lane counts the block's bits of its own run of
entries, five ballots place the runs, the lanes write their entries in order -- copies the block's table rows into its
cube and starts the first batch's loads; an entry present in two consecutive blocks has its partial stored by the one
block's last batch and loaded again by the next block's first.  These cases put the blocks where the list is tightest --
one item (one pose), exactly 64 and 128 items (copies of one pose), one pose among many copies, jobs of a single block (a
receptor of one subtile), jobs of 64 entries (LIGHTDOCK_BM_PART_CAP=64) and the ANM form with wild poses -- and hold the
energies to the oracle's (bm_err) and the in-cutoff pair counts to equality.  LIGHTDOCK_BM_PART_CAP is read at every call,
so it stays set for the whole test; the LIGHTDOCK_BM_DEBUG record's job and block counts show that the cap and the
single-block jobs are in force.
"""
import numpy as np
import pytest

from conftest import case_kwargs, case_positions

pytestmark = pytest.mark.gpu

REL_TOL = 1e-9
BM_ATOL = 1e-11


def bm_err(got, want):
    """The block-major path's error model (tests/test_gpu_parity.py): relative error of what exceeds BM_ATOL."""
    return np.max(np.maximum(np.abs(got - want) - BM_ATOL, 0.0) / np.maximum(np.abs(want), 1e-9))


def _debug_record(monkeypatch, tmp_path, hip, poses):
    """One more call with LIGHTDOCK_BM_DEBUG set: the per-wave records of dfire_bm_pairs (words: 2 jobs, 12 block set-ups)."""
    path = str(tmp_path / "bm_debug.txt")
    monkeypatch.setenv("LIGHTDOCK_BM_DEBUG", path)
    try:
        hip.energy_batch(np.ascontiguousarray(poses))
    finally:
        monkeypatch.delenv("LIGHTDOCK_BM_DEBUG")
    return np.atleast_2d(np.loadtxt(path))


def _energies_and_counts(hip, poses):
    torch = pytest.importorskip("torch")
    n = poses.shape[0]
    dev = torch.device("cuda:0")
    d_poses = torch.from_numpy(np.ascontiguousarray(poses)).to(dev)
    d_out = torch.zeros(n, dtype=torch.float64, device=dev)
    d_cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    hip.energy_batch_device(n, d_poses.data_ptr(), poses.shape[1], d_out.data_ptr(), None, d_cnt.data_ptr())
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_cnt.cpu().numpy().astype(np.int64)


@pytest.fixture(scope="module")
def bm_case(pkg, orc, table):
    """Scorers of a fixture.  (LIGHTDOCK_BM_PART_CAP is read at every call, not when the scorer is built: a test that wants it
    keeps it set for its whole body.)"""
    pkg.init(0)
    cache = {}

    def get(name):
        if name not in cache:
            method, rec, lig, kw = case_kwargs(name, orc, table)
            hip = pkg.Scorer.from_pdb(method, rec, lig, **kw)
            assert hip.kernel_info()["pair_kernel_name"] == "dfire_bm_pairs"
            cache[name] = (hip, orc.Scorer(method, rec, lig, **kw))
        return cache[name]
    return get


def _batches(orc, name):
    poses = case_positions(name, orc)
    return {
        "one pose": poses[:1],                              # every block one item: every batch starts a block
        "two poses": poses[3:5],
        "64 copies": np.repeat(poses[7:8], 64, axis=0),     # blocks of exactly 64 items
        "128 copies": np.repeat(poses[9:10], 128, axis=0),  # ... and of 128: two full batches a block
        "65 copies + 63": np.concatenate([np.repeat(poses[11:12], 65, axis=0), poses[12:75]]),
        "mixed 96": poses[:96],
    }


@pytest.mark.parametrize("part_cap", [None, "64"], ids=["default", "part_cap_64"])
@pytest.mark.parametrize("name", ["1k4c", "1ppe"])
def test_block_boundaries_rigid(bm_case, orc, name, part_cap, monkeypatch, tmp_path):
    hip, cpu = bm_case(name)
    batches = _batches(orc, name)
    if part_cap:
        # the cap is in force: no job holds more than 64 entries, so every block is a single batch (the 128 copies' blocks
        # hold 128 items each where the parts are longer), and there are no fewer jobs than without it
        d_default = _debug_record(monkeypatch, tmp_path, hip, batches["128 copies"])
        monkeypatch.setenv("LIGHTDOCK_BM_PART_CAP", part_cap)
        d_capped = _debug_record(monkeypatch, tmp_path, hip, batches["128 copies"])
        assert d_capped[:, 3].sum() == d_capped[:, 12].sum() > 0, (d_capped[:, 3].sum(), d_capped[:, 12].sum())
        assert d_capped[:, 2].sum() >= d_default[:, 2].sum() > 0
        if name == "1k4c":   # (its 128-entry parts: twice the jobs, two batches a block without the cap)
            assert d_capped[:, 2].sum() >= 1.5 * d_default[:, 2].sum() and d_default[:, 3].sum() > d_default[:, 12].sum()
    for label, poses in batches.items():
        got, cnt = _energies_and_counts(hip, poses)
        uniq, inv = np.unique(poses, axis=0, return_inverse=True)
        want = cpu.energy_rows(uniq)[inv.ravel()]
        stats = np.array([cpu.energy_ex_row(p)[1][5] for p in uniq], dtype=np.int64)[inv.ravel()]
        assert bm_err(got, want) < REL_TOL, (label, part_cap)
        assert np.array_equal(cnt, stats), (label, part_cap)
        if label.endswith("copies"):
            assert np.all(got == got[0]), label   # fixed-point sums: the same pose gives the same bits in every lane


def _write_pdb(path, atoms):
    with open(path, "w") as f:
        for k, (name, res, chain, seq, x, y, z) in enumerate(atoms, 1):
            f.write("ATOM  %5d  %-3s %3s %1s%4d    %8.3f%8.3f%8.3f  1.00  0.00\n" % (k, name, res, chain, seq, x, y, z))


def _molecule(rng, n_atoms, box, chain):
    names = ["N", "CA", "C", "O", "CB", "CG", "CD1", "CD2"]
    return [(names[k % 8], "LEU", chain, 1 + k // 8, *np.round(rng.uniform(-box / 2, box / 2, 3), 3)) for k in range(n_atoms)]


@pytest.mark.parametrize("part_cap", [None, "64"], ids=["default", "part_cap_64"])
@pytest.mark.parametrize("n_rec,n_lig", [(8, 40), (5, 300), (16, 130)])
def test_jobs_of_one_or_two_blocks(pkg, orc, table, tmp_path, monkeypatch, n_rec, n_lig, part_cap):
    """A receptor of one subtile (8 atoms or fewer): every job is a single block; of two subtiles: at most two."""
    rng = np.random.default_rng(31 * n_rec + n_lig)
    rec, lig = str(tmp_path / "rec.pdb"), str(tmp_path / "lig.pdb")
    _write_pdb(rec, _molecule(rng, n_rec, 8.0, "A"))
    _write_pdb(lig, _molecule(rng, n_lig, 24.0, "B"))
    n = 200
    poses = np.zeros((n, 7))
    poses[:, :3] = rng.uniform(-9, 9, (n, 3))
    q = rng.normal(size=(n, 4))
    poses[:, 3:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    poses[100:164] = poses[5]   # a block of 64 copies and more
    if part_cap:
        monkeypatch.setenv("LIGHTDOCK_BM_PART_CAP", part_cap)
    cpu = orc.Scorer("dfire", rec, lig, potential=table)
    hip = pkg.Scorer.from_pdb("dfire", rec, lig, potential=table)
    assert hip.kernel_info()["pair_kernel_name"] == "dfire_bm_pairs"
    got, cnt = _energies_and_counts(hip, poses)
    assert bm_err(got, cpu.energy_rows(poses)) < REL_TOL, (part_cap, n_rec, n_lig)
    assert np.array_equal(cnt, np.array([cpu.energy_ex_row(p)[1][5] for p in poses], dtype=np.int64)), (part_cap, n_rec, n_lig)
    d = _debug_record(monkeypatch, tmp_path, hip, poses)
    jobs, blocks = d[:, 2].sum(), d[:, 12].sum()
    assert 0 < jobs <= blocks <= jobs * -(-n_rec // 8), (jobs, blocks)   # every job of one block (8 atoms or fewer), of two at most


@pytest.mark.parametrize("part_cap", [None, "64"], ids=["default", "part_cap_64"])
def test_block_boundaries_anm_with_wild_poses(bm_case, orc, part_cap, monkeypatch):
    """The ANM form (2uuy: 10 + 10 modes), whose block set-up also stages the receptor subtile's modes: one pose, copies,
    and amplitudes forty times their size for every fifth pose (wild: the block goes through the exact path)."""
    if part_cap:
        monkeypatch.setenv("LIGHTDOCK_BM_PART_CAP", part_cap)
    hip, cpu = bm_case("2uuy")
    base = case_positions("2uuy", orc)
    wild = base[:40].copy()
    wild[::5, 7:] *= 40.0
    for label, poses in {"one pose": base[:1], "one wild pose": wild[:1], "64 copies": np.repeat(base[2:3], 64, axis=0),
                         "wild 40": wild, "wild copies": np.repeat(wild[5:6], 70, axis=0)}.items():
        got = hip.energy_batch(np.ascontiguousarray(poses))
        want = cpu.energy_rows(poses)
        assert bm_err(got, want) < REL_TOL, (label, part_cap)
