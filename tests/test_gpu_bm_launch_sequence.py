"""The launch sequence of the block-major DFIRE path at the shapes where its folded kernels can go wrong.

An energy launch of ONE pass ends in `dfire_bm_finish` (dfire_bm_gather and pose_energy_finish in one kernel), `dfire_bm_census`
cuts the entries into parts itself while the complex has at most 4 096 tile pairs (no `dfire_bm_plan` in front), and
`dfire_bm_pose` clears the (ligand tile, row) sums a thread per word.  Batches of several passes, counting launches and complexes
of more tile pairs keep `dfire_bm_plan` / `dfire_bm_gather` + `pose_energy_finish`; both sequences must give the same bits.

The complex is small -- a receptor of 150 atoms (3 tiles, the last ragged: 22 atoms; 4 membrane beads; a restraint) and a ligand
of 100 atoms (2 tiles, a restraint) -- so 6 tile pairs, and more than 64 poses give tile pairs of several parts (P = 64): part k
of a tile pair starts at entry k x size.  Row counts 1, 9, 64, 65 and 200 leave the finishing kernel's last wave partly filled
(8 lanes a row, 32 rows a workgroup).  Tolerance: the allowance of test_gpu_parity.py's random-molecule tests (1e-11 of
max(|energy|, 1)); integers and the comparison of the two sequences are equalities.  That a batch of several passes does NOT take
the fused launch is held by the sanitizer build: its stand-in for launch_bm_finish refuses a launch that is not the whole batch
(tests/asan/hip_stub_bm_finish.cpp, driven by host_check's LIGHTDOCK_BM_CHUNK=16 batches)."""
import os

import numpy as np
import pytest

from test_gpu_gso_shapes import _against_oracle
from test_gpu_parity import _counts_of, _random_molecule, _random_protein_pdb, _write_pdb

pytestmark = pytest.mark.gpu

ATOL = 1e-11        # of max(|energy|, 1): test_random_molecules_match_oracle's allowance
BM = "dfire_bm_pairs"
N_POSES = 200
FAR = 0             # the pose whose every atom is beyond the cutoff


def _err(got, want):
    return np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0))


def _with_env(env, make):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return make()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _poses(rng, n, cols=7):
    poses = np.zeros((n, cols))
    poses[:, :3] = rng.uniform(-22, 22, (n, 3))
    poses[1:9, :3] = rng.uniform(-2, 2, (8, 3))                # overlapping: clashes, interface flags, beads touched
    q = rng.normal(size=(n, 4))
    poses[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (n, 1))   # non-unit too
    poses[FAR, :3] = (500.0, -300.0, 200.0)
    return poses


def small_complex(rng, table, directory):
    """The files of the complex, drawn from `rng`, and the arguments both Scorer constructors take: (rec, lig, kw)."""
    rec, lig = os.path.join(directory, "rec.pdb"), os.path.join(directory, "lig.pdb")
    rec_atoms = _random_molecule(rng, 146, 28.0, "A", with_beads=4)
    lig_atoms = _random_molecule(rng, 100, 18.0, "B")
    assert len(rec_atoms) == 150 and len(lig_atoms) == 100
    _write_pdb(rec, rec_atoms)
    _write_pdb(lig, lig_atoms)
    return rec, lig, dict(rec_active=["A.%s.%d" % (rec_atoms[0][1], rec_atoms[0][3])],
                          lig_active=["B.%s.%d" % (lig_atoms[-1][1], lig_atoms[-1][3])], potential=table)


def small_anm_kw(rng, kw):
    """`kw` with 3 + 3 modes drawn from `rng`."""
    return dict(kw, use_anm=True, rec_num_anm=3, lig_num_anm=3,
                rec_nmodes=(rng.normal(size=(3, 150, 3)) * 0.4).ravel(), lig_nmodes=(rng.normal(size=(3, 100, 3)) * 0.4).ravel())


class Small:
    """The complex, its poses and the oracle's answers, made once."""

    def __init__(self, pkg, orc, table, directory):
        self.pkg, self.orc, self.table = pkg, orc, table
        rng = np.random.default_rng(4242)
        self.rec, self.lig, self.kw = small_complex(rng, table, directory)
        self.poses = _poses(rng, N_POSES)
        self.cpu = orc.Scorer("dfire", self.rec, self.lig, **self.kw)
        self.hip = pkg.Scorer.from_pdb("dfire", self.rec, self.lig, **self.kw)
        ex = [self.cpu.energy_ex_row(p) for p in self.poses]
        self.want = np.array([e for e, _ in ex], dtype=np.float64)
        self.stats = np.array([s for _, s in ex])
        self.want.setflags(write=False)
        self.stats.setflags(write=False)
        # molecules that flex: 3 + 3 modes, one wild pose
        mrng = np.random.default_rng(4243)
        self.anm_kw = small_anm_kw(mrng, self.kw)
        self.anm_poses = _poses(mrng, 30, 13)
        self.anm_poses[:, 7:] = mrng.normal(size=(30, 6)) * 2.0
        self.anm_poses[5, 7:] *= 40.0


@pytest.fixture(scope="module")
def small(pkg, orc, table, tmp_path_factory):
    pkg.init(0)
    return Small(pkg, orc, table, str(tmp_path_factory.mktemp("bm_launch_sequence")))


def test_the_shape_is_what_the_folds_need(small):
    assert small.hip.kernel_info()["pair_kernel_name"] == BM
    assert small.hip.num_atoms(0) == 150 and small.hip.num_atoms(1) == 100
    s = small.stats
    # the tail's three terms all occur (src/dfire.rs:347-361): receptor restraint, ligand restraint, membrane beads
    assert (s[:, 2] > 0).any() and (s[:, 3] > 0).any() and (s[:, 4] > 0).any(), s[:12, 2:5]
    assert (s[:, 4] == 0).any()
    assert s[FAR, 5] == 0 and small.want[FAR] == 4.7          # no pair inside the cutoff: the tail alone
    assert (s[:, 5] > 0).sum() > 64, "tile pairs of more than 64 entries: several parts"


@pytest.mark.parametrize("n", [1, 9, 64, 65, 200])
def test_single_pass_energies(small, n):
    got = small.hip.energy_batch(small.poses[:n])
    err = _err(got, small.want[:n])
    print("n = %d: %.2e" % (n, err))
    assert err < ATOL
    assert got[FAR] == 4.7
    assert np.array_equal(got, small.hip.energy_batch(small.poses[:n]))   # the part list is the scan's order: the same every launch


@pytest.mark.parametrize("n", [65, 200])
def test_fused_launch_equals_the_unfused_sequences_bit_for_bit(small, n):
    """The same scorer through the counting sequence (dfire_bm_gather + pose_energy_finish), and a scorer of passes of 16 poses on
    two streams: the energies are the fused launch's, ==."""
    torch = pytest.importorskip("torch")
    fused = small.hip.energy_batch(small.poses[:n])
    counted, _ = _counts_of(torch, small.hip, small.poses[:n])
    assert np.array_equal(counted, fused)
    chunked = _with_env({"LIGHTDOCK_BM_CHUNK": "16"}, lambda: small.pkg.Scorer.from_pdb("dfire", small.rec, small.lig, **small.kw))
    assert chunked.kernel_info()["pair_kernel_name"] == BM
    assert np.array_equal(chunked.energy_batch(small.poses[:n]), fused)


def test_passes_of_16_poses_on_two_sets(small):
    """LIGHTDOCK_BM_CHUNK=16 with 50 poses: four passes (16, 16, 16, 2) alternating between two workspace sets: the unfused path."""
    chunked = _with_env({"LIGHTDOCK_BM_CHUNK": "16"}, lambda: small.pkg.Scorer.from_pdb("dfire", small.rec, small.lig, **small.kw))
    assert chunked.kernel_info()["pair_kernel_name"] == BM
    got = chunked.energy_batch(small.poses[:50])
    err = _err(got, small.want[:50])
    print("4 passes: %.2e" % err)
    assert err < ATOL
    assert np.array_equal(got, small.hip.energy_batch(small.poses[:50]))


def test_pair_counts_wanted(small):
    """The counting sequence in front of the energies: in-cutoff pair counts and energies are the oracle's."""
    torch = pytest.importorskip("torch")
    got, counts = _counts_of(torch, small.hip, small.poses[:65])
    assert np.array_equal(counts.astype(np.int64), small.stats[:65, 5].astype(np.int64))
    assert _err(got, small.want[:65]) < ATOL


def test_active_mask_leaves_the_other_energies_alone(small):
    """ld_scorer_energy_batch_device with a mask and no counts: the fused launch writes the active poses' energies only."""
    torch = pytest.importorskip("torch")
    n = 65
    dev = torch.device("cuda:0")
    d_poses = torch.from_numpy(np.ascontiguousarray(small.poses[:n])).to(dev)
    d_out = torch.full((n,), -12345.0, dtype=torch.float64, device=dev)
    active = np.ones(n, dtype=np.uint8)
    active[::3] = 0
    d_active = torch.from_numpy(active).to(dev)
    small.hip.set_stream(torch.cuda.current_stream().cuda_stream)
    small.hip.energy_batch_device(n, d_poses.data_ptr(), 7, d_out.data_ptr(), d_active.data_ptr(), None)
    torch.cuda.synchronize()
    small.hip.set_stream(0)
    out, on = d_out.cpu().numpy(), active == 1
    assert np.all(out[~on] == -12345.0)
    assert np.array_equal(out[on], small.hip.energy_batch(small.poses[:n])[on])


def test_anm_form(small):
    """3 + 3 modes, one wild pose (every block through the exact path): against the oracle, and the counting sequence's bits."""
    torch = pytest.importorskip("torch")
    cpu = small.orc.Scorer("dfire", small.rec, small.lig, **small.anm_kw)
    hip = small.pkg.Scorer.from_pdb("dfire", small.rec, small.lig, **small.anm_kw)
    assert hip.kernel_info()["pair_kernel_name"] == BM
    want = cpu.energy_rows(small.anm_poses)
    got = hip.energy_batch(small.anm_poses)
    err = _err(got, want)
    print("ANM 3 + 3: %.2e" % err)
    assert err < ATOL
    counted, counts = _counts_of(torch, hip, small.anm_poses)
    assert np.array_equal(counted, got)
    assert np.array_equal(counts.astype(np.int64), np.array([cpu.energy_ex_row(p)[1][5] for p in small.anm_poses]).astype(np.int64))


@pytest.mark.parametrize("n_glowworms", [9, 65])
def test_gso_pose_list_form(small, n_glowworms):
    """A GSO's steps evaluate the glowworms that moved, through the compacted list and its device-side count: a live swarm of 9 / 65
    glowworms against the oracle step by step, beside a swarm in which nothing ever moves."""
    live = small.pkg.synth.swarm(n_glowworms, seed=n_glowworms)
    live[:, :3] *= 0.5                                          # near the receptor: energies that differ, neighbours, movement
    still = np.repeat(live[2][None], n_glowworms, axis=0)
    gso = small.pkg.GSO(small.hip, np.stack([live, still]))
    refs = [small.orc.GSO(small.cpu, live), small.orc.GSO(small.cpu, still)]
    moved = 0
    for step in range(1, 6):
        gso.step()
        for s, ref in enumerate(refs):
            ref.step()
            _against_oracle(small.hip, gso.read(s), ref.state(), "%d glowworms, swarm %d, step %d" % (n_glowworms, s, step))
        moved += int(gso.read(0)["moved"].sum())
    assert moved > 0, "the live swarm should move"
    assert gso.num_evals == refs[0].num_evals + refs[1].num_evals
    assert not gso.read(1)["moved"].any() and np.array_equal(gso.read(1)["poses"], still)


def test_gso_step_without_a_job(small):
    """Swarms whose glowworms share one pose: after the first step nothing moves, the list is empty, the launch has no job
    (dfire_bm_order lists none), and the energies stay what they were."""
    still = np.repeat(small.poses[3][None], 9, axis=0)
    quiet = small.pkg.GSO(small.hip, np.stack([still, still]))
    quiet.step()
    before = [quiet.read(s)["scoring"].copy() for s in range(2)]
    evals = quiet.num_evals
    for _ in range(3):
        quiet.step()
    assert quiet.num_evals == evals == 2 * 9
    for s in range(2):
        assert np.array_equal(quiet.read(s)["scoring"], before[s])
    assert _err(before[0], np.repeat(small.want[3], 9)) < ATOL


@pytest.mark.parametrize("n_rec,plans", [(16384, True), (16385, False)])
def test_tile_pairs_at_the_bound_of_the_census_plan(pkg, orc, table, tmp_path, n_rec, plans):
    """A ligand of 16 tiles against a receptor of 256 tiles (4 096 tile pairs: dfire_bm_census plans for itself, its LDS array
    full) and of 257 (4 112: dfire_bm_plan runs in front, as before)."""
    rec, lig = str(tmp_path / "rec.pdb"), str(tmp_path / "lig.pdb")
    _random_protein_pdb(rec, n_rec, 5, 47.0)
    _random_protein_pdb(lig, 1024, 6, 12.0)
    hip = pkg.Scorer.from_pdb("dfire", rec, lig, potential=table)
    cpu = orc.Scorer("dfire", rec, lig, potential=table)
    assert hip.kernel_info()["pair_kernel_name"] == BM
    assert (-(-hip.num_atoms(0) // 64) * -(-hip.num_atoms(1) // 64) <= 4096) == plans
    poses = pkg.synth.swarm(12, seed=31)
    poses[:, :3] *= 0.8
    got = hip.energy_batch(poses)
    err = _err(got, cpu.energy_rows(poses))
    print("%d x 16 tile pairs: %.2e" % (-(-n_rec // 64), err))
    assert err < ATOL
    assert np.array_equal(got, hip.energy_batch(poses))
