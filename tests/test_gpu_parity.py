"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C ABI,
against the CPU oracle on the same inputs, against the reference's committed outputs
(tests/golden), and through size-independent properties at full batch sizes.

Tolerances.  BASELINE.json's north star asks for 1e-4 relative on energies and exact
glowworm indices.  Every DECISION a pair takes -- cutoff, distance bin, interface flag -- is the
reference's f64 decision bit for bit: the DNA / PYDOCK and all-f64 DFIRE kernels do their geometry in
f64 in the reference's operation order; the default DFIRE kernels (block-major `dfire_bm_*`, pose-major
`dfire_packed_pairs`) reach the same decisions through an f32 filter whose every doubtful pair is
redone in f64 (the in-cutoff pair COUNT of a pose is asserted equal to the
oracle's).  What differs from the CPU is the SUM: its order (f64 kernels: `rel_err`, ~1e-13 observed)
or, on the block-major path, 64-bit fixed-point table values rounded once to 2^-40 (`bm_err`: an
absolute error model, 2-7e-12 observed).  We hold the energies to REL_TOL = 1e-9 and everything
integer to equality.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, case_kwargs, case_positions, parse_gso

pytestmark = pytest.mark.gpu

REL_TOL = 1e-9          # energies, vs the oracle (north star allows 1e-4)
NORTH_STAR_TOL = 1e-4


def rel_err(got, want):
    """Relative error (values below 1e-9 are measured against 1e-9).  For every path whose sums are f64: DNA / PYDOCK, the
    pose-major DFIRE kernels (ANM complexes, LIGHTDOCK_DFIRE_KERNEL=packed | allpairs), K2's luciferins of those."""
    return np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-9))


BM_ATOL = 1e-11


def bm_err(got, want):
    """Error of energies that come from the block-major DFIRE path (dfire_bm_pairs: DFIRE with rigid molecules): relative
    error of what exceeds BM_ATOL.  That path sums table values as 64-bit fixed point, every value rounded ONCE to
    2^-(44-e) (2^e >= the table's largest |value|; 2^-40 for the synthetic table) and added exactly, in any order: an
    ABSOLUTE error model, |err| <= N_pairs * 2^-(45-e) * 0.0157 (src/dfire.rs:347) -- below 8e-10 for 1k4c's 114 k pairs
    in the worst case, 2-4e-12 observed (tools/err_probe.py) -- whatever the size of the energy, which is
    4.7 - 0.0157 * sum and passes through zero.  BM_ATOL = 1e-11 is an EMPIRICAL allowance, two to five times what is observed and far
    below the model's worst case: a legitimate worst-case batch could exceed it and would have to be judged against the model
    (bench.py derives its allowance from the model: P_cut * 2^-(45-e) * 0.0157 per pose).  Where the fixed point is held
    EXACTLY -- at every scale exponent e and extra bit x, against integer arithmetic, to the roundings of the tail -- is
    tests/test_gpu_dfire_tables.py; this measure stays what it was for the tests here."""
    return np.max(np.maximum(np.abs(got - want) - BM_ATOL, 0.0) / np.maximum(np.abs(want), 1e-9))


BM_DFIRE = ("1ppe", "1k4c", "2uuy", "ab_icode")   # the DFIRE fixtures: the block-major path by default (2uuy, ab_icode: its ANM form)


def err_for(name, env=None):
    """The error measure of a fixture's default K1 (or of the kernel `env` forces; LIGHTDOCK_TILED_LATENCY=1: the pose-major one)."""
    env = env or {}
    kernel = env.get("LIGHTDOCK_DFIRE_KERNEL", "packed" if env.get("LIGHTDOCK_TILED_LATENCY") else "bm")
    return bm_err if name in BM_DFIRE and kernel == "bm" else rel_err


@pytest.fixture(scope="module")
def scorers(pkg, orc, table):
    pkg.init(0)
    cache = {}

    def get(name):
        if name not in cache:
            method, rec, lig, kw = case_kwargs(name, orc, table)
            cache[name] = (pkg.Scorer.from_pdb(method, rec, lig, **kw), orc.Scorer(method, rec, lig, **kw))
        return cache[name]
    return get


def test_native_library_is_loaded(pkg):
    lib = pkg.load_library()
    assert pkg.device_count() >= 1
    maps = open("/proc/self/maps").read()
    assert "liblightdock_hip.so" in maps
    assert lib.ld_init(0) == 0


@pytest.mark.parametrize("name,n", [("1ppe", 200), ("1k4c", 200), ("2uuy", 120), ("ab_icode", 60), ("1azp", 200)])
def test_pose_energies_match_oracle(scorers, orc, name, n):
    """K1 over the reference's starting poses: DFIRE (+restraint, +membrane, +ANM) and DNA+ANM."""
    hip, cpu = scorers(name)
    poses = case_positions(name, orc)[:n]
    got = hip.energy_batch(poses)
    want = cpu.energy_rows(poses)
    assert err_for(name)(got, want) < REL_TOL
    assert err_for(name)(got, want) < NORTH_STAR_TOL


def test_dna_known_answer_and_reference_goldens(pkg, scorers, orc):
    """The reference's own numbers: src/dna.rs:571 and example/1azp/swarm_0/gso_1.out."""
    d = os.path.join(GOLDEN, "unit", "1azp")
    s = pkg.Scorer.from_pdb("dna", os.path.join(d, "1azp_receptor.pdb"), os.path.join(d, "1azp_ligand.pdb"))
    e = s.energy([0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0])
    assert abs(e - (-364.88126358158974)) < 1e-10 * 364.9
    hip, _ = scorers("1azp")
    poses = case_positions("1azp", orc)
    _, _, _, _, sco = parse_gso(os.path.join(GOLDEN, "1azp", "swarm_0", "gso_1.out"))
    got = hip.energy_batch(poses)
    assert np.all(np.abs(got - sco) <= 0.51e-8 + 1e-11 * np.abs(sco))      # 8 printed decimals


def test_membrane_and_restraint_tails_are_exercised(scorers, orc):
    """1k4c starting poses touch membrane beads (penalty 999 * fraction, src/dfire.rs:355-359);
    1ppe has an active receptor restraint (src/dfire.rs:350-353)."""
    hip, cpu = scorers("1k4c")
    poses = case_positions("1k4c", orc)
    stats = np.array([cpu.energy_ex_row(p)[1] for p in poses[:60]])
    assert (stats[:, 4] > 0).sum() >= 3, "fixture should include membrane-intersecting poses"
    got = hip.energy_batch(poses[:60])
    want = cpu.energy_rows(poses[:60])
    assert bm_err(got, want) < REL_TOL
    hip, cpu = scorers("1ppe")
    poses = case_positions("1ppe", orc)
    stats = np.array([cpu.energy_ex_row(p)[1] for p in poses])
    assert (stats[:, 2] > 0).sum() >= 1, "fixture should satisfy the E.ILE.16 restraint somewhere"


def test_scalar_energy_equals_batch(scorers, orc):
    hip, cpu = scorers("1azp")
    poses = case_positions("1azp", orc)[:4]
    batch = hip.energy_batch(poses)
    for row, want in zip(poses, batch):
        assert hip.energy(row[:3], row[3:7], row[7:17], row[17:27]) == want    # same kernel, same order
    hip, _ = scorers("1ppe")
    poses = case_positions("1ppe", orc)[:4]
    batch = hip.energy_batch(poses)
    for row, want in zip(poses, batch):
        assert hip.energy(row[:3], row[3:7]) == want


def test_construct_from_arrays_equals_from_pdb(pkg, scorers, orc, table):
    """ld_scorer_create (arrays, the FFI a Rust `impl Score` would use) == ld_scorer_create_from_pdb."""
    hip, cpu = scorers("1ppe")
    s2 = pkg.Scorer.from_arrays("dfire", cpu.model(0), cpu.model(1), potential=table)
    poses = case_positions("1ppe", orc)[:32]
    assert np.array_equal(s2.energy_batch(poses), hip.energy_batch(poses))
    m = hip.model_arrays(0)
    assert np.array_equal(m["dfire_types"], cpu.model(0)["dfire_types"])


def test_atom_order_invariance(pkg, scorers, orc, table):
    """Summation order is the only liberty the kernel takes: permuting atoms (and remapping the
    restraint / membrane indices) changes energies by rounding only."""
    hip, cpu = scorers("1k4c")
    rng = np.random.default_rng(3)
    models = []
    for side in (0, 1):
        m = cpu.model(side)
        perm = rng.permutation(len(m["dfire_types"]))
        inv = np.empty_like(perm)
        inv[perm] = np.arange(len(perm))
        models.append({"coordinates": m["coordinates"][perm], "dfire_types": m["dfire_types"][perm],
                       "membrane": inv[m["membrane"]].astype(np.uint32), "restraint_offsets": m["restraint_offsets"],
                       "restraint_atoms": inv[m["restraint_atoms"]].astype(np.uint32)})
    s2 = pkg.Scorer.from_arrays("dfire", models[0], models[1], potential=table)
    poses = case_positions("1k4c", orc)[:64]
    assert bm_err(s2.energy_batch(poses), hip.energy_batch(poses)) < REL_TOL


def test_device_batch_active_mask_and_pair_counts(pkg, scorers, orc):
    """ld_scorer_energy_batch_device: poses resident in HBM, `active` bytes skip poses
    (src/glowworm.rs:62), pair_counts = P_cut of the algorithmic-bytes model."""
    torch = pytest.importorskip("torch")
    hip, cpu = scorers("1ppe")
    poses = case_positions("1ppe", orc)[:48]
    dev = torch.device("cuda:0")
    d_poses = torch.from_numpy(poses).to(dev)
    d_out = torch.full((48,), -12345.0, dtype=torch.float64, device=dev)
    active = np.ones(48, dtype=np.uint8)
    active[::3] = 0
    d_active = torch.from_numpy(active).to(dev)
    d_cnt = torch.zeros(48, dtype=torch.int32, device=dev)
    hip.set_stream(torch.cuda.current_stream().cuda_stream)
    hip.energy_batch_device(48, d_poses.data_ptr(), poses.shape[1], d_out.data_ptr(), d_active.data_ptr(), d_cnt.data_ptr())
    torch.cuda.synchronize()
    hip.set_stream(0)
    out, cnt = d_out.cpu().numpy(), d_cnt.cpu().numpy()
    want = cpu.energy_rows(poses)
    on = active == 1
    assert bm_err(out[on], want[on]) < REL_TOL
    assert np.all(out[~on] == -12345.0)
    stats = np.array([cpu.energy_ex_row(p)[1][5] for p in poses])
    assert np.array_equal(cnt[on].astype(np.int64), stats[on].astype(np.int64))


def test_error_paths(pkg, scorers, table):
    hip, _ = scorers("1ppe")
    with pytest.raises(pkg.LightdockError, match="stride"):
        hip.energy_batch(np.zeros((2, 5)))
    with pytest.raises(pkg.LightdockError, match="DFIRE parameters"):
        pkg.Scorer.from_pdb("dfire", os.path.join(GOLDEN, "1ppe", "lightdock_1ppe_e.pdb"),
                            os.path.join(GOLDEN, "1ppe", "lightdock_1ppe_i.pdb"))
    assert hip.energy_batch(np.zeros((0, 7))).shape == (0,)       # empty batch is a no-op


def test_full_size_batch_properties(pkg, scorers, orc):
    """BASELINE-size batch of 1k4c poses (bench.py's 8192, same construction): replicated poses give
    bit-identical energies wherever they sit in the batch (no cross-pose interference, no
    dependence on the workgroup that ran them), and a sample agrees with the oracle."""
    hip, cpu = scorers("1k4c")
    base = case_positions("1k4c", orc)
    n = 8192
    poses = pkg.synth.jitter(base, n, seed=11)
    poses[n // 2:] = poses[:n // 2]                       # second half repeats the first
    e = hip.energy_batch(poses)
    assert np.array_equal(e[:n // 2], e[n // 2:])
    assert np.array_equal(hip.energy_batch(poses[:7]), e[:7])   # independent of batch size
    idx = np.random.default_rng(0).choice(n // 2, size=24, replace=False)
    assert bm_err(e[idx], cpu.energy_rows(poses[idx])) < REL_TOL


def test_batch_larger_than_one_block_major_pass(pkg, scorers, orc):
    """20 000 poses of 1k4c: more than one pass of the block-major path holds (19 456 for this complex's 2 808 tile pairs), so
    the batch runs as two passes, 19 456 + 544, on two streams with two workspace sets -- by the library's own rule, no
    test knob.  Duplicated poses must give the same bits whichever pass evaluates them, and a sample across both passes
    agrees with the oracle."""
    hip, cpu = scorers("1k4c")
    assert hip.kernel_info()["pair_kernel_name"] == "dfire_bm_pairs"
    base = case_positions("1k4c", orc)
    n = 20000
    poses = pkg.synth.jitter(base, n, seed=12)
    poses[n // 2:] = poses[:n // 2]                       # row 10 000 + k repeats row k: 544 of them cross the pass boundary
    e = hip.energy_batch(poses)
    assert np.array_equal(e[:n // 2], e[n // 2:])
    assert np.array_equal(hip.energy_batch(poses[:5]), e[:5])
    idx = np.concatenate([np.random.default_rng(1).choice(n // 2, size=10, replace=False), [19455, 19456, n - 1]])
    assert bm_err(e[idx], cpu.energy_rows(poses[idx])) < REL_TOL


def test_pass_of_more_than_65536_rows(pkg, scorers, orc):
    """70 000 poses of 1ppe are ONE pass of the block-major path (its 104 tile pairs allow 262 144 rows a pass), and a pass of
    more than 2^16 rows is where the pair kernel keeps an entry's row in 16 + 2 bits (the late steps of a GSO over hundreds of
    swarms are such launches).  Duplicates on either side of row 65 536 give the same bits; a sample against the oracle."""
    hip, cpu = scorers("1ppe")
    assert hip.kernel_info()["pair_kernel_name"] == "dfire_bm_pairs"
    n = 70000
    poses = pkg.synth.jitter(case_positions("1ppe", orc), n, seed=21)
    poses[n // 2:] = poses[:n // 2]                       # row 35 000 + k repeats row k: rows 65 536 .. 69 999 repeat 30 536 .. 34 999
    e = hip.energy_batch(poses)
    assert np.array_equal(e[:n // 2], e[n // 2:])
    idx = np.array([0, 30536, 34999, 65535, 65536, 65537, 69999])
    assert bm_err(e[idx], cpu.energy_rows(poses[idx])) < REL_TOL


def test_pass_smaller_than_the_batch_by_construction(pkg, orc, table, tmp_path):
    """A 9 000-atom receptor (141 tiles) against the 3 268-atom ligand of 1k4c (52 tiles): 7 332 tile pairs, for which one
    pass of the block-major path holds 7 168 poses -- a batch of 8 192 (the bench size) is two passes by construction.
    Against the oracle on a sample, duplicates identical across the passes."""
    import time
    rec = str(tmp_path / "big_rec.pdb")
    _random_protein_pdb(rec, 9000, 1, 60.0)
    lig = os.path.join(GOLDEN, "1k4c", "lightdock_ligand.pdb")
    hip = pkg.Scorer.from_pdb("dfire", rec, lig, potential=table)
    cpu = orc.Scorer("dfire", rec, lig, potential=table)
    assert hip.kernel_info()["pair_kernel_name"] == "dfire_bm_pairs"
    n = 8192
    poses = pkg.synth.jitter(case_positions("1k4c", orc), n, seed=13)
    poses[n // 2:] = poses[:n // 2]
    e = hip.energy_batch(poses)
    t0 = time.perf_counter()
    e2 = hip.energy_batch(poses)
    dt = time.perf_counter() - t0
    print("9000 x 3268 atoms, 8192 poses in two passes: %.0f evals/s (host buffers)" % (n / dt))
    assert np.array_equal(e, e2) and np.array_equal(e[:n // 2], e[n // 2:])
    idx = np.array([0, 1, 2047, 4095, 6143, 6144, 8191])
    assert bm_err(e[idx], cpu.energy_rows(poses[idx])) < REL_TOL


@pytest.mark.parametrize("name,steps", [("1ppe", 100), ("1azp", 12), ("1k4c", 6)])
def test_gso_steps_match_oracle(pkg, scorers, orc, name, steps):
    """K1 + K2 step by step against the oracle's GSO: neighbour counts, chosen neighbour ids and
    moved flags exact AT EVERY STEP; luciferin / vision / scoring / poses to rounding.  1ppe runs the reference's full length
    (100 steps, src/lib.rs:46-58; tools/long_run_check.py is the 400-step version).  1k4c is the headline
    system: the block-major K1 fed by K2's compacted list of the glowworms that moved, 52 ligand tiles, the membrane penalty
    (src/dfire.rs:355-359) on some of the swarm's poses."""
    hip, cpu = scorers(name)
    poses = case_positions(name, orc)
    if name == "1k4c":
        bead_hits = np.array([cpu.energy_ex_row(p)[1][4] for p in poses])
        assert (bead_hits > 0).sum() >= 3, "the swarm should hold membrane-penalised poses"
    gso = pkg.GSO(hip, poses)
    ref = orc.GSO(cpu, poses)
    for step in range(1, steps + 1):
        gso.step()
        ref.step()
        a, b = gso.read(0), ref.state()
        assert np.array_equal(a["n_neighbors"], b["n_neighbors"]), "step %d" % step
        assert np.array_equal(a["target"], b["target"]), "step %d" % step
        assert np.array_equal(a["moved"], b["moved"]), "step %d" % step
        assert err_for(name)(a["scoring"], b["scoring"]) < REL_TOL
        assert err_for(name)(a["luciferin"], b["luciferin"]) < REL_TOL
        assert np.array_equal(a["vision_range"], b["vision_range"])
        assert np.max(np.abs(a["poses"] - b["poses"])) < 1e-12
    assert gso.num_evals == ref.num_evals
    assert gso.steps_done == steps


def test_gso_reproduces_reference_files_1azp(pkg, scorers, orc, tmp_path):
    """20 steps of the real example (DNA + ANM + restraints) against the files the Rust binary
    wrote (example/1azp/swarm_0/gso_{1,10,20}.out): integers exact, reals to print precision."""
    hip, _ = scorers("1azp")
    gso = pkg.GSO(hip, case_positions("1azp", orc))        # default seed 324324, src/constants.rs:2
    for step in range(1, 21):
        gso.step()
        if step in (1, 10, 20):
            gso.save(0, step, str(tmp_path))
            got = parse_gso(os.path.join(tmp_path, "gso_%d.out" % step))
            want = parse_gso(os.path.join(GOLDEN, "1azp", "swarm_0", "gso_%d.out" % step))
            assert np.array_equal(got[2], want[2])                              # neighbour counts
            assert np.max(np.abs(got[0] - want[0])) <= 1.01e-7                  # coordinates, 7 decimals
            assert np.max(np.abs(got[3] - want[3])) <= 1.01e-3                  # vision range, 3 decimals
            assert np.all(np.abs(got[1] - want[1]) <= 1.01e-8 + 1e-9 * np.abs(want[1]))   # luciferin
            assert np.all(np.abs(got[4] - want[4]) <= 1.01e-8 + 1e-9 * np.abs(want[4]))   # scoring
    header = open(os.path.join(tmp_path, "gso_1.out")).readline()
    assert header == "#Coordinates  RecID  LigID  Luciferin  Neighbor's number  Vision Range  Scoring\n"


def test_gso_many_swarms_are_independent(pkg, scorers, orc):
    """Swarms never exchange data (src/bin/lightdock-rust.rs:171-188): a batch of swarms equals
    each swarm run alone; equal swarms with equal seeds stay equal, different seeds diverge."""
    hip, cpu = scorers("1ppe")
    base = case_positions("1ppe", orc)[:64]
    other = pkg.synth.swarm(64, seed=5)
    batch = np.stack([base, other, base, base])
    seeds = np.array([324324, 324324, 324324, 99], dtype=np.uint64)
    gso = pkg.GSO(hip, batch, seeds=seeds)
    refs = [orc.GSO(cpu, batch[s], seed=int(seeds[s])) for s in range(4)]
    for _ in range(15):
        gso.step()
        for r in refs:
            r.step()
    for s in range(4):
        a, b = gso.read(s), refs[s].state()
        assert np.array_equal(a["n_neighbors"], b["n_neighbors"]) and np.array_equal(a["target"], b["target"])
        assert bm_err(a["luciferin"], b["luciferin"]) < REL_TOL
    a0, a2, a3 = gso.read(0), gso.read(2), gso.read(3)
    assert np.array_equal(a0["poses"], a2["poses"]) and np.array_equal(a0["luciferin"], a2["luciferin"])
    assert not np.array_equal(a0["target"], a3["target"])


def test_gso_step_in_which_nothing_moves(pkg, scorers, orc):
    """Late in a run whole swarms sit still: a swarm whose glowworms share one pose has no neighbours (luciferins equal,
    src/glowworm.rs:104), so a step evaluates nothing -- the block-major kernels of such a step are launched with zero rows and
    leave before their set-up.  Next to it a live swarm, whose steps must not notice."""
    hip, cpu = scorers("1ppe")
    base = case_positions("1ppe", orc)[:64]
    still = np.repeat(base[3][None], 64, axis=0)
    gso = pkg.GSO(hip, np.stack([still, base, still]))
    quiet = pkg.GSO(hip, np.stack([still, still]))
    refs = [orc.GSO(cpu, still), orc.GSO(cpu, base)]
    for _ in range(6):
        gso.step()
        quiet.step()
        for r in refs:
            r.step()
    evals_after_start = quiet.num_evals
    quiet.step()
    assert quiet.num_evals == evals_after_start == 2 * 64   # step 0 scores every glowworm once; nothing since
    for s, r in ((0, refs[0]), (1, refs[1]), (2, refs[0])):
        a, b = gso.read(s), r.state()
        assert np.array_equal(a["n_neighbors"], b["n_neighbors"]) and np.array_equal(a["target"], b["target"])
        assert np.array_equal(a["moved"], b["moved"])
        assert bm_err(a["scoring"], b["scoring"]) < REL_TOL and bm_err(a["luciferin"], b["luciferin"]) < REL_TOL
        assert np.max(np.abs(a["poses"] - b["poses"])) < 1e-12
    assert not gso.read(0)["moved"].any() and np.array_equal(gso.read(0)["poses"], still)
    assert np.array_equal(quiet.read(0)["scoring"], quiet.read(1)["scoring"])


def test_cli_end_to_end_1azp(pkg, tmp_path):
    """The reference command line on the GPU engine: same stdout lines, same files
    (src/bin/lightdock-rust.rs:158-333)."""
    src = os.path.join(GOLDEN, "1azp")
    for f in ("rec_nm.npy", "lig_nm.npy"):
        shutil.copy(os.path.join(src, f), tmp_path)
    r = subprocess.run([pkg.CLI_PATH, os.path.join(src, "setup.json"), os.path.join(src, "initial_positions_0.dat"),
                        "10", "dna"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0].startswith("Reading starting positions from \"") and lines[1] == "Swarm ID 0"
    assert lines[2] == "Writing to swarm dir \"swarm_0\""
    assert "Loading DNA scoring function" in lines and "Creating GSO with 200 glowworms" in lines
    assert lines[-1] == "Starting optimization (10 steps)"
    assert "Output directory does not exist for swarm 0, creating it" in r.stderr
    for step in (1, 10):
        got = parse_gso(os.path.join(tmp_path, "swarm_0", "gso_%d.out" % step))
        want = parse_gso(os.path.join(src, "swarm_0", "gso_%d.out" % step))
        assert np.array_equal(got[2], want[2])
        assert np.max(np.abs(got[0] - want[0])) <= 1.01e-7
        assert np.all(np.abs(got[4] - want[4]) <= 1.01e-8 + 1e-9 * np.abs(want[4]))
    assert not os.path.exists(os.path.join(tmp_path, "swarm_0", "gso_5.out"))     # only 1 and every 10th


def test_cli_dfire_with_synthetic_table(pkg, orc, table, tmp_path):
    """BASELINE config 1/2: 1ppe DFIRE through both CLIs (oracle CPU path vs HIP path) with the
    synthetic DCparams in ./data, files compared numerically."""
    src = os.path.join(GOLDEN, "1ppe")
    for name in ("cpu", "gpu"):
        os.makedirs(os.path.join(tmp_path, name, "data"))
        pkg.synth.write_dcparams(os.path.join(tmp_path, name, "data", "DCparams"), table)
    args = [os.path.join(src, "setup.json"), os.path.join(src, "initial_positions_0.dat"), "20", "dfire"]
    orc.lib()
    r1 = subprocess.run([orc.CLI_PATH] + args, cwd=os.path.join(tmp_path, "cpu"), capture_output=True, text=True)
    r2 = subprocess.run([pkg.CLI_PATH] + args, cwd=os.path.join(tmp_path, "gpu"), capture_output=True, text=True)
    assert r1.returncode == 0 and r2.returncode == 0, r1.stderr + r2.stderr
    assert r1.stdout == r2.stdout
    for step in (1, 10, 20):
        a = parse_gso(os.path.join(tmp_path, "cpu", "swarm_0", "gso_%d.out" % step))
        b = parse_gso(os.path.join(tmp_path, "gpu", "swarm_0", "gso_%d.out" % step))
        assert np.array_equal(a[2], b[2])
        assert np.max(np.abs(a[0] - b[0])) <= 1.01e-7
        assert np.all(np.abs(a[4] - b[4]) <= 1.01e-8 + 1e-9 * np.abs(a[4]))


def test_real_dcparams_goldens_on_gpu(pkg, orc, real_dcparams):
    """Opt-in: with the real table the HIP path must hit src/dfire.rs:415 and example/1ppe gso_1.out."""
    t = pkg.load_dcparams(real_dcparams)
    d = os.path.join(GOLDEN, "unit", "2oob")
    s = pkg.Scorer.from_pdb("dfire", os.path.join(d, "2oob_receptor.pdb"), os.path.join(d, "2oob_ligand.pdb"), potential=t)
    assert abs(s.energy([0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]) - 16.7540569503498) < 1e-11


@pytest.mark.parametrize("env", [
    {"LIGHTDOCK_DFIRE_KERNEL": "allpairs"},
    {"LIGHTDOCK_DFIRE_KERNEL": "tiled"},      # no such kernel any more: an unknown value, the default route
    {"LIGHTDOCK_TILED_LATENCY": "1"},         # the single-swarm CLI's setting: the pose-major kernel, split 3 below 32 ligand tiles
    {"LIGHTDOCK_TILED_LATENCY": "1", "LIGHTDOCK_DFIRE_KERNEL": "bm"},     # ... with the block-major path forced
    {"LIGHTDOCK_DFIRE_KERNEL": "packed"},                                  # the pose-major kernel (what ANM runs use)
    {"LIGHTDOCK_DFIRE_KERNEL": "packed", "LIGHTDOCK_PACKED_CELLS": "2"},    # ... with half-unit LUT cells
    {"LIGHTDOCK_DFIRE_KERNEL": "packed", "LIGHTDOCK_PACKED_EPS_SCALE": "8"},
    {"LIGHTDOCK_PACKED_EPS_SCALE": "8"},      # a wider error band: more pairs on the exact path, same results
    {"LIGHTDOCK_BM_CHUNK": "16"},             # block-major passes of 16 poses, alternating between two streams
    {"LIGHTDOCK_BM_CHUNK": "16", "LIGHTDOCK_BM_LANES": "1"},
    {"LIGHTDOCK_BM_ANM": "0"},                # molecules that flex stay with the pose-major kernel
    {"LIGHTDOCK_BM_PART_CAP": "64"},          # jobs of 64 entries: every block a single batch, every entry's sum through many jobs
    {"LIGHTDOCK_TILED_SPLIT": "2"},
])
@pytest.mark.parametrize("name", ["1ppe", "1k4c", "2uuy"])
def test_dfire_kernel_variants_agree(pkg, orc, table, scorers, name, env):
    """The all-pairs kernel, the pose-major packed-f32 kernel and the default block-major path (both: box culling + f32 pair
    test with exact f64 path, in several settings, and as the environment picks them) are routes to the same sum: all match
    the oracle, and the in-cutoff pair counts -- which neither culling nor the f32 test may change by a single pair -- are
    identical."""
    torch = pytest.importorskip("torch")
    default_hip, cpu = scorers(name)
    method, rec, lig, kw = case_kwargs(name, orc, table)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        variant = pkg.Scorer.from_pdb(method, rec, lig, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    poses = case_positions(name, orc)[:64]
    want = cpu.energy_rows(poses)
    assert err_for(name, env)(variant.energy_batch(poses), want) < REL_TOL
    dev = torch.device("cuda:0")
    d_poses = torch.from_numpy(poses).to(dev)
    counts = []
    for s in (variant, default_hip):
        d_out = torch.zeros(64, dtype=torch.float64, device=dev)
        d_cnt = torch.zeros(64, dtype=torch.int32, device=dev)
        s.energy_batch_device(64, d_poses.data_ptr(), poses.shape[1], d_out.data_ptr(), None, d_cnt.data_ptr())
        torch.cuda.synchronize()
        counts.append(d_cnt.cpu().numpy())
    assert np.array_equal(counts[0], counts[1])
    stats = np.array([cpu.energy_ex_row(p)[1][5] for p in poses[:16]])
    assert np.array_equal(counts[0][:16].astype(np.int64), stats.astype(np.int64))


@pytest.mark.parametrize("kernel", [{}, {"LIGHTDOCK_DFIRE_KERNEL": "packed"}, {"LIGHTDOCK_DFIRE_KERNEL": "packed", "LIGHTDOCK_PACKED_CELLS": "2"}])
@pytest.mark.parametrize("name", ["1ppe", "1k4c", "2uuy"])
@pytest.mark.parametrize("zeroed", [(19,), (17, 18, 19), (5, 19), (0, 1, 19)])
def test_bins_that_are_zero_for_the_whole_complex_are_not_read(pkg, orc, table, name, zeroed, kernel, monkeypatch):
    """A potential that is 0.0 in a bin for every type pair of the complex (DFIRE's reference state does
    that to the last shell) lets the default kernel skip the table for the pairs of that bin.  The sums
    must equal those of the same kernel reading the zeros (to rounding: the pairs that go through the
    exact path are folded by other lanes when the queue holds fewer of them), the oracle must agree, and
    the in-cutoff pair counts still count every pair."""
    torch = pytest.importorskip("torch")
    t = table.copy()
    for b in zeroed:
        t.reshape(169, 169, 20)[:, :, b] = 0.0
    method, rec, lig, kw = case_kwargs(name, orc, t)
    for k, v in kernel.items():
        monkeypatch.setenv(k, v)
    skipping = pkg.Scorer.from_pdb(method, rec, lig, **kw)
    monkeypatch.setenv("LIGHTDOCK_PACKED_ELIDE_ZERO_BINS", "0")
    reading = pkg.Scorer.from_pdb(method, rec, lig, **kw)
    monkeypatch.delenv("LIGHTDOCK_PACKED_ELIDE_ZERO_BINS")
    cpu = orc.Scorer(method, rec, lig, **kw)
    poses = case_positions(name, orc)[:64]
    got = skipping.energy_batch(poses)
    assert err_for(name, kernel)(got, reading.energy_batch(poses)) < 1e-12
    assert err_for(name, kernel)(got, cpu.energy_rows(poses)) < REL_TOL
    dev = torch.device("cuda:0")
    d_poses = torch.from_numpy(poses).to(dev)
    counts = []
    for s in (skipping, reading):
        d_out = torch.zeros(64, dtype=torch.float64, device=dev)
        d_cnt = torch.zeros(64, dtype=torch.int32, device=dev)
        s.energy_batch_device(64, d_poses.data_ptr(), poses.shape[1], d_out.data_ptr(), None, d_cnt.data_ptr())
        torch.cuda.synchronize()
        counts.append(d_cnt.cpu().numpy())
        assert err_for(name, kernel)(d_out.cpu().numpy(), got) < 1e-12     # the counting launch reads the full LUT: same sums again
    assert np.array_equal(counts[0], counts[1])
    stats = np.array([cpu.energy_ex_row(p)[1][5] for p in poses[:8]])
    assert np.array_equal(counts[0][:8].astype(np.int64), stats.astype(np.int64))


def test_gso_run_graph_replay_equals_stepping(pkg, scorers, orc, monkeypatch):
    """ld_gso_run with LIGHTDOCK_GSO_GRAPH=1 (captured hipGraph, two steps per replay) == ld_gso_step repeated == oracle."""
    monkeypatch.setenv("LIGHTDOCK_GSO_GRAPH", "1")
    hip, cpu = scorers("1ppe")
    poses = case_positions("1ppe", orc)
    a, b = pkg.GSO(hip, poses), pkg.GSO(hip, poses)
    a.run(25)                 # eager + graph replays + odd tail
    a.step()                  # odd number of eager steps after the capture ...
    a.run(9)                  # ... then replay again
    for _ in range(35):
        b.step()
    ref = orc.GSO(cpu, poses)
    for _ in range(35):
        ref.step()
    sa, sb, sr = a.read(0), b.read(0), ref.state()
    assert a.steps_done == 35 and b.steps_done == 35
    for k in ("poses", "luciferin", "vision_range", "scoring", "n_neighbors", "target", "moved"):
        assert np.array_equal(sa[k], sb[k]), k
    assert np.array_equal(sa["target"], sr["target"]) and np.array_equal(sa["n_neighbors"], sr["n_neighbors"])
    assert a.num_evals == b.num_evals == ref.num_evals


def test_dna_coincident_atoms_score_nan_like_the_reference(pkg, orc, tmp_path):
    """Two atoms on the same spot: src/dna.rs:498-503 computes p6 = R^6 / 0 = inf, k = e * (inf - inf) = NaN,
    and its ordered compare `k > VDW_CUTOFF` keeps the NaN, so the score is NaN (the oracle agrees).  The
    kernel clamps with fmin/fmax, which drop NaNs, and must put it back."""
    rec, lig = str(tmp_path / "r.pdb"), str(tmp_path / "l.pdb")
    _write_pdb(rec, [("N", "ALA", "A", 1, 0.0, 0.0, 0.0), ("CA", "ALA", "A", 1, 1.4, 0.3, 0.0)])
    _write_pdb(lig, [("N", "GLY", "B", 1, 0.0, 0.0, 0.0), ("CA", "GLY", "B", 1, 3.0, 0.0, 0.0)])
    hip, cpu = pkg.Scorer.from_pdb("dna", rec, lig), orc.Scorer("dna", rec, lig)
    poses = np.array([[0, 0, 0, 1, 0, 0, 0], [0.5, 0, 0, 1, 0, 0, 0]], dtype=np.float64)
    want, got = cpu.energy_rows(poses), hip.energy_batch(poses)
    assert np.isnan(want[0]) and np.isnan(got[0])
    assert np.isfinite(want[1]) and abs(got[1] - want[1]) <= 1e-9 * abs(want[1])


@pytest.mark.parametrize("cells", ["1", "2"])
def test_atoms_outside_the_f32_frame_take_the_exact_path(pkg, orc, table, cells, monkeypatch):
    """The default DFIRE kernel keeps f32 records in a frame around the receptor; atoms outside it (absurd
    ANM extents here: coefficients of hundreds of angstroms) are flagged and every pair of theirs is
    decided in f64 -- through the per-wave queue or, when that overflows, the all-f64 pass of the wave.
    Energies and in-cutoff pair counts must still equal the oracle's."""
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("LIGHTDOCK_PACKED_CELLS", cells)
    method, rec, lig, kw = case_kwargs("2uuy", orc, table)
    hip, cpu = pkg.Scorer.from_pdb(method, rec, lig, **kw), orc.Scorer(method, rec, lig, **kw)
    poses = case_positions("2uuy", orc)[:24].copy()
    rng = np.random.default_rng(9)
    poses[:8, 7:17] *= 400.0                                  # receptor modes: atoms fly out of the frame
    poses[8:16, 17:27] *= 400.0                               # ligand modes
    poses[16:20, :3] += rng.normal(0.0, 300.0, size=(4, 3))   # ligand far away: nothing in range
    want = np.array([cpu.energy_ex_row(p) for p in poses], dtype=object)
    want_e = np.array([w[0] for w in want], dtype=np.float64)
    want_n = np.array([w[1][5] for w in want]).astype(np.int64)
    dev = torch.device("cuda:0")
    d_poses = torch.from_numpy(poses).to(dev)
    d_out = torch.zeros(len(poses), dtype=torch.float64, device=dev)
    d_cnt = torch.zeros(len(poses), dtype=torch.int32, device=dev)
    hip.energy_batch_device(len(poses), d_poses.data_ptr(), poses.shape[1], d_out.data_ptr(), None, d_cnt.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d_cnt.cpu().numpy().astype(np.int64), want_n)
    assert rel_err(d_out.cpu().numpy(), want_e) < REL_TOL
    assert rel_err(hip.energy_batch(poses), want_e) < REL_TOL
    assert want_n[:16].max() > 0 and np.all(want_n[16:20] == 0)


def test_gso_graph_survives_workspace_reallocation(pkg, scorers, orc, monkeypatch):
    """The captured hipGraph carries the addresses of the scorer's shared workspaces.  A larger batch
    on the same scorer reallocates them between two ld_gso_run calls: the next run must capture
    again instead of replaying launches into freed memory."""
    monkeypatch.setenv("LIGHTDOCK_GSO_GRAPH", "1")
    hip, cpu = scorers("1ppe")
    poses = case_positions("1ppe", orc)
    a, b = pkg.GSO(hip, poses), pkg.GSO(hip, poses)
    a.run(12)                                             # captures at 200 poses
    big = np.tile(poses, (40, 1))
    hip.energy_batch(big)                                 # 8000 poses: every workspace grows
    big_gso = pkg.GSO(hip, np.stack([poses] * 24))        # and a larger GSO on the same scorer
    big_gso.run(8)
    a.run(12)
    for _ in range(24):
        b.step()
    sa, sb = a.read(0), b.read(0)
    for k in ("poses", "luciferin", "vision_range", "scoring", "n_neighbors", "target", "moved"):
        assert np.array_equal(sa[k], sb[k]), k
    assert a.num_evals == b.num_evals


def _write_pdb(path, atoms):
    """atoms: (name, resname, chain, resseq, x, y, z)"""
    with open(path, "w") as f:
        for k, (name, res, chain, seq, x, y, z) in enumerate(atoms, 1):
            f.write("ATOM  %5d  %-3s %3s %1s%4d    %8.3f%8.3f%8.3f  1.00  0.00\n" % (k, name, res, chain, seq, x, y, z))


def test_tiny_molecules_and_cutoff_corners(pkg, orc, table, tmp_path):
    """Edge cases of src/dfire.rs:325-345 on hand-made molecules, every DFIRE kernel variant:
    r = 15.0 A exactly (inclusive cutoff, reads bin 20 = next row's bin 0), r < 0.5 A (negative d
    saturates to index 0), an interface pair (d <= 3.9), ligand/receptor far smaller than a tile,
    a pose that leaves no pair in range (score = 4.7), non-unit quaternions (src/qt.rs:48-50)."""
    rec = str(tmp_path / "rec.pdb")
    lig = str(tmp_path / "lig.pdb")
    _write_pdb(rec, [("N", "ALA", "A", 1, 0.0, 0.0, 0.0), ("CA", "ALA", "A", 1, 1.4, 0.3, 0.0),
                     ("BJ", "MMB", "C", 9, -3.0, 0.0, 0.0), ("OH", "TYR", "A", 2, 0.0, 4.0, 1.0)])
    _write_pdb(lig, [("N", "GLY", "B", 1, 15.0, 0.0, 0.0), ("CA", "GLY", "B", 1, 0.05, 0.05, 0.05),
                     ("SG", "CYS", "B", 2, -3.5, 1.2, 0.0)])
    poses = np.array([
        [0, 0, 0, 1, 0, 0, 0],                      # identity: r = 15 exactly for (rec N, lig N)
        [0, 0, 0, 2.0, 0, 0, 0],                    # same rotation, quaternion of norm 2
        [100.0, 0, 0, 1, 0, 0, 0],                  # nothing in range
        [0.5, -0.25, 0.125, 0.5, 0.5, 0.5, 0.5],    # 120 degree rotation about (1,1,1)
        [1e-3, 0, 0, 0.9, 0.1, -0.3, 0.2],
    ], dtype=np.float64)
    cpu = orc.Scorer("dfire", rec, lig, rec_active=["A.TYR.2"], lig_active=["B.CYS.2"], potential=table)
    e0, st0 = cpu.energy_ex_row(poses[0])
    assert st0[5] >= 3 and st0[4] > 0            # in-cutoff pairs incl. the r = 15 one; the bead is touched
    assert cpu.energy_row(poses[2]) == 4.7
    want = cpu.energy_rows(poses)
    assert want[0] == want[1]
    for env in ({}, {"LIGHTDOCK_DFIRE_KERNEL": "allpairs"}, {"LIGHTDOCK_TILED_SPLIT": "2"}):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            hip = pkg.Scorer.from_pdb("dfire", rec, lig, rec_active=["A.TYR.2"], lig_active=["B.CYS.2"], potential=table)
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        got = hip.energy_batch(poses)
        assert bm_err(got, want) < 1e-12, env
        assert got[2] == 4.7


_RES_ATOMS = {"ALA": ["N", "CA", "C", "O", "CB"], "GLY": ["N", "CA", "C", "O"], "SER": ["N", "CA", "C", "O", "CB", "OG"],
              "LEU": ["N", "CA", "C", "O", "CB", "CG", "CD1", "CD2"], "LYS": ["N", "CA", "C", "O", "CB", "CG", "CD", "CE", "NZ"],
              "ASP": ["N", "CA", "C", "O", "CB", "CG", "OD1", "OD2"], "PHE": ["N", "CA", "C", "O", "CB", "CG", "CD1", "CD2", "CE1", "CE2", "CZ"]}


def _random_molecule(rng, n_atoms, box, chain, with_beads=0):
    """n_atoms atoms of random residues at uniform positions in a cube (dense: many pairs in every
    distance bin, atoms of one residue far apart, i.e. loose subtile boxes); `with_beads` membrane
    beads on top."""
    atoms, seq = [], 1
    names = sorted(_RES_ATOMS)
    while len(atoms) < n_atoms:
        res = names[int(rng.integers(len(names)))]
        for a in _RES_ATOMS[res]:
            if len(atoms) < n_atoms:
                x, y, z = np.round(rng.uniform(-box / 2, box / 2, 3), 3)
                atoms.append((a, res, chain, seq, x, y, z))
        seq += 1
    for _ in range(with_beads):
        x, y, z = np.round(rng.uniform(-box / 2, box / 2, 3), 3)
        atoms.append(("BJ", "MMB", "M", seq, x, y, z))
        seq += 1
    return atoms


@pytest.mark.parametrize("n_rec,n_lig", [(1, 1), (9, 7), (64, 8), (65, 63), (200, 130), (513, 65), (1100, 300)])
def test_random_molecules_match_oracle(pkg, orc, table, tmp_path, n_rec, n_lig):
    """Seeded random molecules around the tile / subtile / ballot size boundaries (1, 8, 64 atoms,
    one more, one less), random poses incl. overlapping ones, with restraints and membrane beads:
    DFIRE on both kernels, and the all-pairs DNA kernel on the same geometry is covered by the
    fixtures.  Energies against the oracle at 1e-11 of the summed magnitude."""
    rng = np.random.default_rng(1000 * n_rec + n_lig)
    rec, lig = str(tmp_path / "rec.pdb"), str(tmp_path / "lig.pdb")
    rec_atoms = _random_molecule(rng, n_rec, 28.0, "A", with_beads=3 if n_rec >= 64 else 0)
    lig_atoms = _random_molecule(rng, n_lig, 18.0, "B")
    _write_pdb(rec, rec_atoms)
    _write_pdb(lig, lig_atoms)
    rec_active = ["A.%s.%d" % (rec_atoms[0][1], rec_atoms[0][3])]
    lig_active = ["B.%s.%d" % (lig_atoms[-1][1], lig_atoms[-1][3])]
    poses = np.zeros((24, 7))
    poses[:, :3] = rng.uniform(-22, 22, (24, 3))
    poses[:4, :3] = rng.uniform(-2, 2, (4, 3))                 # overlapping: clashes, interface flags
    q = rng.normal(size=(24, 4))
    poses[:, 3:] = q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (24, 1))   # non-unit too
    cpu = orc.Scorer("dfire", rec, lig, rec_active=rec_active, lig_active=lig_active, potential=table)
    want = cpu.energy_rows(poses)
    scale = np.maximum(np.abs(want), 1.0)
    for env in ({}, {"LIGHTDOCK_DFIRE_KERNEL": "allpairs"}):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            hip = pkg.Scorer.from_pdb("dfire", rec, lig, rec_active=rec_active, lig_active=lig_active, potential=table)
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        got = hip.energy_batch(poses)
        assert np.max(np.abs(got - want) / scale) < 1e-11, (env, n_rec, n_lig)


@pytest.mark.parametrize("n_rec,n_lig,k_rec,k_lig", [(9, 7, 2, 3), (64, 8, 10, 0), (65, 63, 0, 10), (200, 130, 10, 10), (513, 65, 7, 1), (1100, 300, 10, 10)])
def test_random_molecules_with_normal_modes_match_oracle(pkg, orc, table, tmp_path, n_rec, n_lig, k_rec, k_lig):
    """The same with molecules that flex (src/dfire.rs:288-320): random modes, amplitudes of a few angstroms and, for a tenth
    of the poses, forty times that (WILD for the block-major path's ANM form: everything through the exact path).  The default
    kernel and the all-pairs kernel against the oracle; `tools/fuzz_parity.py <cases> <seed> anm` is the long form of this."""
    rng = np.random.default_rng(7000 * n_rec + n_lig)
    rec, lig = str(tmp_path / "rec.pdb"), str(tmp_path / "lig.pdb")
    rec_atoms = _random_molecule(rng, n_rec, 28.0, "A", with_beads=3 if n_rec >= 64 else 0)
    lig_atoms = _random_molecule(rng, n_lig, 18.0, "B")
    _write_pdb(rec, rec_atoms)
    _write_pdb(lig, lig_atoms)
    n = 30
    poses = np.zeros((n, 7 + k_rec + k_lig))
    poses[:, :3] = rng.uniform(-22, 22, (n, 3))
    poses[:4, :3] = rng.uniform(-2, 2, (4, 3))
    q = rng.normal(size=(n, 4))
    poses[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (n, 1))
    poses[:, 7:] = rng.normal(size=(n, k_rec + k_lig)) * 2.0
    poses[::10, 7:] *= 40.0
    kw = dict(rec_active=["A.%s.%d" % (rec_atoms[0][1], rec_atoms[0][3])], lig_active=["B.%s.%d" % (lig_atoms[-1][1], lig_atoms[-1][3])],
              potential=table, use_anm=True, rec_num_anm=k_rec, lig_num_anm=k_lig,
              rec_nmodes=(rng.normal(size=(k_rec, len(rec_atoms), 3)) * 0.4).ravel() if k_rec else None,
              lig_nmodes=(rng.normal(size=(k_lig, len(lig_atoms), 3)) * 0.4).ravel() if k_lig else None)
    cpu = orc.Scorer("dfire", rec, lig, **kw)
    want = cpu.energy_rows(poses)
    scale = np.maximum(np.abs(want), 1.0)
    for env in ({}, {"LIGHTDOCK_DFIRE_KERNEL": "allpairs"}):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            hip = pkg.Scorer.from_pdb("dfire", rec, lig, **kw)
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        if not env:
            assert hip.kernel_info()["pair_kernel_name"] == "dfire_bm_pairs"
        got = hip.energy_batch(poses)
        assert np.max(np.abs(got - want) / scale) < 1e-11, (env, n_rec, n_lig)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("name", ["1ppe", "1azp"])
def test_degenerate_poses_neither_hang_nor_poison_the_batch(scorers, orc, name):
    """NaN / infinite translations and a zero quaternion (rotate divides by |q|^2, src/qt.rs:48-50)
    give garbage energies in the reference too; here they must not hang a kernel, and the valid
    poses of the same batch must keep their exact energies."""
    hip, cpu = scorers(name)
    poses = case_positions(name, orc)[:12].copy()
    good = hip.energy_batch(poses)
    bad = poses.copy()
    bad[1, 0] = np.nan
    bad[3, :3] = [np.inf, -np.inf, 1e308]
    bad[5, 3:7] = 0.0
    bad[7, :3] = 1e15
    got = hip.energy_batch(bad)
    keep = [0, 2, 4, 6, 8, 9, 10, 11]
    assert np.array_equal(got[keep], good[keep])
    far = cpu.energy_row(bad[7])
    assert got[7] == far                                   # nothing in range: the same constant as the CPU path
    assert np.array_equal(hip.energy_batch(poses), good)   # and the scorer is still usable


K2_SHAPES = [None, "single", "phased"]   # LIGHTDOCK_GSO_K2: the launch's own choice, gso_movement_phase, gso_movement_phased


def _k2_env(monkeypatch, shape):
    if shape is None:
        monkeypatch.delenv("LIGHTDOCK_GSO_K2", raising=False)
    else:
        monkeypatch.setenv("LIGHTDOCK_GSO_K2", shape)


def test_gso_odd_sizes(pkg, scorers, orc, monkeypatch):
    """1 glowworm (never has a neighbour), 3 glowworms, swarms around the 256 glowworms up to which K2 keeps a bit per candidate
    for the roulette, a swarm of more glowworms than a workgroup has threads (1030 > 1024: one swarm is split over 17 workgroups with
    shares of 61, so no thread here takes a second glowworm -- shares larger than a workgroup are tests/test_gpu_gso_shapes.py's), a
    swarm whose LDS snapshot exceeds 64 KiB (2048: exactly 64 KiB for the thread-per-glowworm
    kernel, 96 KiB for the phased one; 2100): same as the oracle, in BOTH shapes of K2 (src/swarm.rs:72-126; the launch picks
    one by size, gso_step.hip, LIGHTDOCK_GSO_K2 forces one), and the two shapes' states bit for bit the same."""
    hip, cpu = scorers("1ppe")
    base = case_positions("1ppe", orc)
    # (65, 130, 256: inside the kernels' kept-verdict range -- one, three and four words of bits --, 257: just beyond it)
    for n, steps in ((1, 3), (3, 5), (65, 6), (130, 6), (256, 5), (257, 5), (1030, 3), (2048, 2), (2100, 2)):
        pos = pkg.synth.jitter(base, n, seed=n) if n > 200 else base[:n]
        ref = orc.GSO(cpu, pos)
        for _ in range(steps):
            ref.step()
        b = ref.state()
        states = []
        for shape in K2_SHAPES:
            _k2_env(monkeypatch, shape)
            gso = pkg.GSO(hip, pos)
            for _ in range(steps):
                gso.step()
            a = gso.read(0)
            assert np.array_equal(a["n_neighbors"], b["n_neighbors"]) and np.array_equal(a["target"], b["target"]), (n, shape)
            assert np.array_equal(a["moved"], b["moved"]), (n, shape)
            assert bm_err(a["luciferin"], b["luciferin"]) < REL_TOL
            assert np.array_equal(a["vision_range"], b["vision_range"])
            assert gso.num_evals == ref.num_evals
            states.append(a)
        for other in states[1:]:
            for k in ("poses", "luciferin", "scoring", "vision_range", "n_neighbors", "target", "moved"):
                assert np.array_equal(states[0][k], other[k]), (n, k)
    monkeypatch.delenv("LIGHTDOCK_GSO_K2", raising=False)
    g = pkg.GSO(hip, base[:4])
    g.run(0)
    assert g.steps_done == 0 and g.num_evals == 0
    st = g.read(0)
    assert np.all(st["luciferin"] == 5.0) and np.all(st["vision_range"] == 0.2) and np.all(st["moved"] == 0)


@pytest.mark.parametrize("shape", K2_SHAPES)
def test_gso_many_swarms_in_both_k2_shapes(pkg, scorers, orc, monkeypatch, shape):
    """The same batch of swarms through either shape of K2: 96 swarms x 200 glowworms and 6 x 64 (both inside the phased
    kernel's own range of 65 536 glowworms: `single` is what gets forced) and 520 x 200 (104 000: beyond it, `phased` forced)
    -- sampled swarms equal the oracle, replicated swarms stay bit-identical."""
    _k2_env(monkeypatch, shape)
    hip, cpu = scorers("1ppe")
    base = case_positions("1ppe", orc)
    for n_swarms, n, steps, sample in ((96, 200, 5, (0, 41, 95)), (6, 64, 8, (0, 1, 5)), (520, 200, 3, (0, 519))):
        swarms = [base[:n]] + [pkg.synth.swarm(n, seed=100 + k) for k in range(1, n_swarms)]
        swarms[n_swarms - 1] = swarms[1]
        gso = pkg.GSO(hip, np.stack(swarms))
        gso.run(steps)
        a, b = gso.read(1), gso.read(n_swarms - 1)
        for k in ("poses", "luciferin", "scoring", "n_neighbors", "target"):
            assert np.array_equal(a[k], b[k]), k
        for s in sample:
            ref = orc.GSO(cpu, swarms[s])
            for _ in range(steps):
                ref.step()
            st, want = gso.read(s), ref.state()
            assert np.array_equal(st["n_neighbors"], want["n_neighbors"]) and np.array_equal(st["target"], want["target"])
            assert np.array_equal(st["moved"], want["moved"])
            assert bm_err(st["scoring"], want["scoring"]) < REL_TOL and bm_err(st["luciferin"], want["luciferin"]) < REL_TOL
            assert np.max(np.abs(st["poses"] - want["poses"])) < 1e-12


def test_gso_dfire_with_anm_2uuy(pkg, scorers, orc):
    """DFIRE with receptor + ligand ANM (per-pose receptor image, src/dfire.rs:304-320) inside
    the GSO loop, incl. the ANM move step (src/glowworm.rs:159-188)."""
    hip, cpu = scorers("2uuy")
    assert hip.kernel_info()["pair_kernel_name"] == "dfire_bm_pairs"     # the block-major path's ANM form: `bm_err` is its measure
    poses = case_positions("2uuy", orc)[:96]
    gso, ref = pkg.GSO(hip, poses), orc.GSO(cpu, poses)
    for step in range(1, 41):   # (tools/long_run_check_anm.py is the 200-step version)
        gso.step()
        ref.step()
        a, b = gso.read(0), ref.state()
        assert np.array_equal(a["n_neighbors"], b["n_neighbors"]), "step %d" % step
        assert np.array_equal(a["target"], b["target"]), "step %d" % step
        assert np.array_equal(a["moved"], b["moved"]), "step %d" % step
        assert err_for("2uuy")(a["scoring"], b["scoring"]) < REL_TOL
        assert np.max(np.abs(a["poses"] - b["poses"])) < 1e-12
    assert gso.num_evals == ref.num_evals


def test_library_before_torch_shares_one_hip_runtime():
    """Loading the HIP library before PyTorch must not leave two HIP runtimes in the process
    (torch would then report no GPU): tools/check_load_order.py runs smoke(), then imports
    torch, runs an op and lists the libamdhip64 copies mapped."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([os.sys.executable, os.path.join(root, "tools", "check_load_order.py")], capture_output=True,
                       text=True, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "smoke ok" in r.stdout and "cuda available True" in r.stdout and "torch op 140.0" in r.stdout
    mapped = r.stdout.split("hip runtimes mapped:")[1]
    assert mapped.count("libamdhip64") == 1, mapped


def test_receptor_anm_batch_slicing(pkg, scorers, orc, tmp_path):
    """With receptor ANM every pose carries its own receptor image; very large batches are cut
    into slices so that workspace stays bounded.  A child process with the bound lowered to
    1 MiB (a handful of poses per slice) must return bit-identical energies."""
    hip, _ = scorers("2uuy")
    poses = case_positions("2uuy", orc)
    want = hip.energy_batch(poses)
    np.save(tmp_path / "poses.npy", poses)
    code = (
        "import sys, os, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import __graft_entry__ as ge\n"
        "from conftest import case_kwargs\n"
        "import torch; torch.cuda.init()\n"
        "pkg, orc = ge.package(), ge.oracle(); pkg.init(0)\n"
        "m, rec, lig, kw = case_kwargs('2uuy', orc, pkg.synth.dcparams())\n"
        "s = pkg.Scorer.from_pdb(m, rec, lig, **kw)\n"
        "np.save(%r, s.energy_batch(np.load(%r)))\n"
    ) % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)),
         str(tmp_path / "sliced.npy"), str(tmp_path / "poses.npy"))
    env = dict(os.environ, LIGHTDOCK_RECEPTOR_IMAGE_MIB="1")
    r = subprocess.run([os.sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(np.load(tmp_path / "sliced.npy"), want)


def test_receptor_anm_with_more_modes_than_the_image_kernel_keeps_in_registers(pkg, orc, table):
    """The receptor-image kernel keeps 10 modes per atom in registers and reads any further ones per
    pose; the exact path deforms its atoms by the same operations.  13 receptor modes, odd batch sizes
    (the kernel takes 16 poses per wave), an active mask with holes, and a widened error band so that
    hundreds of pairs go through the exact path."""
    torch = pytest.importorskip("torch")
    method, rec, lig, kw = case_kwargs("2uuy", orc, table)
    rng = np.random.default_rng(11)
    rec_modes = np.asarray(kw["rec_nmodes"], dtype=np.float64).reshape(10, -1)
    extra = 0.05 * rng.standard_normal((3, rec_modes.shape[1]))
    kw["rec_nmodes"] = np.concatenate([rec_modes, extra]).reshape(-1)
    kw["rec_num_anm"] = 13
    base = case_positions("2uuy", orc)
    poses = np.concatenate([base[:, :17], rng.uniform(-1.0, 1.0, (len(base), 3)), base[:, 17:]], axis=1)[:83]
    cpu = orc.Scorer(method, rec, lig, **kw)
    want = cpu.energy_rows(poses)
    for env in ({}, {"LIGHTDOCK_PACKED_EPS_SCALE": "8"}):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            hip = pkg.Scorer.from_pdb(method, rec, lig, **kw)
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        assert rel_err(hip.energy_batch(poses), want) < REL_TOL
        assert rel_err(hip.energy_batch(poses[:17]), want[:17]) < REL_TOL
        dev = torch.device("cuda:0")
        d_poses = torch.from_numpy(poses).to(dev)
        active = (np.arange(len(poses)) % 3 != 1).astype(np.uint8)
        d_active = torch.from_numpy(active).to(dev)
        d_out = torch.full((len(poses),), 7.0, dtype=torch.float64, device=dev)
        hip.energy_batch_device(len(poses), d_poses.data_ptr(), poses.shape[1], d_out.data_ptr(), d_active.data_ptr())
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert rel_err(got[active == 1], want[active == 1]) < REL_TOL
        assert np.all(got[active == 0] == 7.0)


@pytest.mark.timeout(900)
def test_cli_100_steps_matches_reference_files_1azp(pkg, tmp_path):
    """The full published run of the example: 100 steps, all 11 gso files against the files the
    Rust binary wrote (example/1azp/swarm_0)."""
    src = os.path.join(GOLDEN, "1azp")
    for f in ("rec_nm.npy", "lig_nm.npy"):
        shutil.copy(os.path.join(src, f), tmp_path)
    r = subprocess.run([pkg.CLI_PATH, os.path.join(src, "setup.json"), os.path.join(src, "initial_positions_0.dat"),
                        "100", "dna"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for step in [1] + list(range(10, 101, 10)):
        got = parse_gso(os.path.join(tmp_path, "swarm_0", "gso_%d.out" % step))
        want = parse_gso(os.path.join(src, "swarm_0", "gso_%d.out" % step))
        assert np.array_equal(got[2], want[2]), "neighbour counts differ at step %d" % step
        assert np.max(np.abs(got[0] - want[0])) <= 1.01e-7
        assert np.max(np.abs(got[3] - want[3])) <= 1.01e-3
        assert np.all(np.abs(got[1] - want[1]) <= 1.01e-8 + 1e-9 * np.abs(want[1]))
        assert np.all(np.abs(got[4] - want[4]) <= 1.01e-8 + 1e-9 * np.abs(want[4]))


def test_pydock_method(pkg, orc, scorers, tmp_path):
    """Method::PYDOCK (src/scoring.rs:5-9): DNA's energy behind the pydock model builder."""
    d = os.path.join(GOLDEN, "unit", "1azp")
    rec, lig = os.path.join(d, "1azp_receptor.pdb"), os.path.join(d, "1azp_ligand.pdb")
    s = pkg.Scorer.from_pdb("pydock", rec, lig)
    assert abs(s.energy([0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]) - (-364.88126358158974)) < 1e-10 * 364.9   # src/pydock.rs:586
    odd = tmp_path / "odd.pdb"
    odd.write_text("ATOM      1  CQ1 LIG A   1       1.104   3.207   2.100  1.00  0.00           C\n"
                   "ATOM      2  F7  LIG A   1       2.104   3.207   2.100  1.00  0.00           F\n"
                   "ATOM      3  S1  LIG A   1       2.104   4.207   2.100  1.00  0.00           S\n")
    hip, cpu = pkg.Scorer.from_pdb("pydock", str(odd), lig), orc.Scorer("pydock", str(odd), lig)
    poses = np.array([[0, 0, 0, 1, 0, 0, 0], [3.0, -2.0, 1.0, 0.5, 0.5, -0.5, 0.5]], dtype=np.float64)
    assert rel_err(hip.energy_batch(poses), cpu.energy_rows(poses)) < REL_TOL
    # the CLI accepts the third method name; the mode files are given in lightdock's own
    # (modes, atoms, 3) shape (lightdock_*.nm.npy) instead of lgd_flatten's flat one
    src = os.path.join(GOLDEN, "1azp")
    for f, atoms in (("rec_nm.npy", 1094), ("lig_nm.npy", 506)):
        np.save(tmp_path / f, np.load(os.path.join(src, f)).reshape(10, atoms, 3))
    r = subprocess.run([pkg.CLI_PATH, os.path.join(src, "setup.json"), os.path.join(src, "initial_positions_0.dat"),
                        "1", "PyDock"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0 and "Loading PYDOCK scoring function" in r.stdout
    got = parse_gso(os.path.join(tmp_path, "swarm_0", "gso_1.out"))
    want = parse_gso(os.path.join(src, "swarm_0", "gso_1.out"))          # identical to the DNA run
    assert np.all(np.abs(got[4] - want[4]) <= 1.01e-8 + 1e-9 * np.abs(want[4]))


def test_c_example_client(pkg, tmp_path):
    """examples/dna_energy.c: a plain C program against include/lightdock_hip.h reproduces the
    reference's DNA known answer (src/dna.rs:571) and runs a batch."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "dna_energy"
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", pkg.INCLUDE_DIR,
                        os.path.join(root, "examples", "dna_energy.c"), "-L", lib_dir, "-llightdock_hip",
                        "-Wl,-rpath," + lib_dir, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    d = os.path.join(GOLDEN, "unit", "1azp")
    r = subprocess.run([str(exe), os.path.join(d, "1azp_receptor.pdb"), os.path.join(d, "1azp_ligand.pdb")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert abs(float(lines[0].split(":")[1]) - (-364.88126358158974)) < 1e-10 * 364.9
    assert len(lines) == 5 and abs(float(lines[1].split(":")[1]) - float(lines[0].split(":")[1])) < 1e-9   # x = 0 again


def test_multi_swarm_launcher(pkg, tmp_path):
    """launch.py (the ant_thony.py replacement): three swarms in one batched GSO write the same
    files as three runs of the single-swarm CLI."""
    src = os.path.join(GOLDEN, "1azp")
    run, init = tmp_path / "run", tmp_path / "init"
    run.mkdir(), init.mkdir()
    for f in ("rec_nm.npy", "lig_nm.npy"):
        shutil.copy(os.path.join(src, f), run)
    base = open(os.path.join(src, "initial_positions_0.dat")).read().splitlines()
    for s, shift in ((0, 0), (1, 60), (2, 120)):
        (init / ("initial_positions_%d.dat" % s)).write_text("\n".join(base[shift:shift + 64]) + "\n")
    launcher = os.path.join(os.path.dirname(pkg.__file__), "launch.py")
    r = subprocess.run([os.sys.executable, launcher, os.path.join(src, "setup.json"), "12", "dna", "--swarms", "0-2",
                        "--init-dir", str(init)], cwd=run, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for s in range(3):
        single = tmp_path / ("single%d" % s)
        single.mkdir()
        for f in ("rec_nm.npy", "lig_nm.npy"):
            shutil.copy(os.path.join(src, f), single)
        r = subprocess.run([pkg.CLI_PATH, os.path.join(src, "setup.json"), str(init / ("initial_positions_%d.dat" % s)),
                            "12", "dna"], cwd=single, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        for step in (1, 10):
            a = open(run / ("swarm_%d" % s) / ("gso_%d.out" % step)).read()
            b = open(single / ("swarm_%d" % s) / ("gso_%d.out" % step)).read()
            assert a == b
        assert not os.path.exists(run / ("swarm_%d" % s) / "gso_12.out")
    # the same three swarms sharded over two ranks (one process per GPU under torchrun; both ranks
    # share device 0 here): rank 0 takes swarms 0 and 2, rank 1 swarm 1; same files
    run2 = tmp_path / "run2"
    run2.mkdir()
    for f in ("rec_nm.npy", "lig_nm.npy"):
        shutil.copy(os.path.join(src, f), run2)
    env = dict(os.environ, LIGHTDOCK_DEVICE="0")
    r = subprocess.run([os.sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", "29533", launcher, os.path.join(src, "setup.json"), "12", "dna",
                        "--swarms", "0-2", "--init-dir", str(init)], cwd=run2, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "rank 0/2: 2 swarms" in r.stdout and "rank 1/2: 1 swarms" in r.stdout
    for s in range(3):
        for step in (1, 10):
            name = os.path.join("swarm_%d" % s, "gso_%d.out" % step)
            assert open(run2 / name).read() == open(run / name).read()


@pytest.mark.timeout(600)
def test_launcher_on_the_reference_multi_swarm_example_1czy(pkg, orc, tmp_path):
    """example/1czy is the reference's only real multi-swarm run (example/1czy/execution.sh:20-24: ten
    `lightdock-rust setup.json init/initial_positions_<i>.dat 100 dfire` tasks under ant_thony.py):
    DFIRE + receptor/ligand ANM + an active receptor restraint, 1281 x 53 atoms.  launch.py does the ten
    swarms as one batched GSO; every gso_*.out must equal what the CPU oracle CLI writes for the
    same swarm to print precision, neighbour counts exactly (synthetic DCparams: the real table is
    not in the reference mount).
    The ANM modes are read from lightdock_{rec,lig}.nm.npy as lightdock3_setup.py leaves them."""
    src = os.path.join(GOLDEN, "1czy")
    run = tmp_path / "run"
    (run / "data").mkdir(parents=True)
    pkg.synth.write_dcparams(str(run / "data" / "DCparams"))
    for f in ("lightdock_rec.nm.npy", "lightdock_lig.nm.npy"):      # no flattened rec_nm.npy / lig_nm.npy here
        shutil.copy(os.path.join(src, f), run)
    launcher = os.path.join(os.path.dirname(pkg.__file__), "launch.py")
    steps = 20
    r = subprocess.run([os.sys.executable, launcher, os.path.join(src, "setup.json"), str(steps), "dfire", "--swarms", "0-9",
                        "--init-dir", os.path.join(src, "init")], cwd=run, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "10 swarms" in r.stdout
    ref = tmp_path / "ref"
    (ref / "data").mkdir(parents=True)
    shutil.copy(run / "data" / "DCparams", ref / "data" / "DCparams")
    for f in ("rec_nm.npy", "lig_nm.npy"):                           # the reference's own flattened files
        shutil.copy(os.path.join(src, f), ref)
    for s in (0, 3, 9):
        r = subprocess.run([orc.CLI_PATH, os.path.join(src, "setup.json"), os.path.join(src, "init", "initial_positions_%d.dat" % s),
                            str(steps), "dfire"], cwd=ref, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        for step in (1, 10, 20):
            name = os.path.join("swarm_%d" % s, "gso_%d.out" % step)
            a, b = parse_gso(str(run / name)), parse_gso(str(ref / name))
            assert np.array_equal(a[2], b[2]), name                    # neighbour counts
            for x, y in zip(a, b):
                assert np.allclose(x, y, rtol=0, atol=2e-7), name      # print precision (7 / 8 decimals)
    for s in range(10):
        assert sorted(os.listdir(run / ("swarm_%d" % s))) == ["gso_1.out", "gso_10.out", "gso_20.out"]


def test_gso_save_many_equals_save_and_reports_errors(pkg, scorers, orc, tmp_path):
    """ld_gso_save_many (one device read, files written by threads) writes what ld_gso_save writes swarm by
    swarm; n = 0 is a no-op; a swarm index out of range and an unwritable directory are errors."""
    hip, _ = scorers("1ppe")
    poses = case_positions("1ppe", orc)
    gso = pkg.GSO(hip, np.stack([poses[:64], poses[64:128], poses[128:192]]))
    gso.run(10)
    one, many = tmp_path / "one", tmp_path / "many"
    for s in range(3):
        (one / str(s)).mkdir(parents=True)
        (many / str(s)).mkdir(parents=True)
        gso.save(s, 10, str(one / str(s)))
    gso.save_many([2, 0, 1], 10, [str(many / "2"), str(many / "0"), str(many / "1")])
    for s in range(3):
        assert open(one / str(s) / "gso_10.out").read() == open(many / str(s) / "gso_10.out").read()
    gso.save_many([], 10, [])
    with pytest.raises(pkg.LightdockError):
        gso.save_many([3], 10, [str(many / "0")])
    with pytest.raises(pkg.LightdockError):
        gso.save_many([0], 10, [str(tmp_path / "missing" / "dir")])


def test_block_count_diagnostics(pkg, scorers, orc):
    """The culled kernel evaluates far fewer 8x8 blocks than all pairs, never fewer than the
    in-cutoff pairs need."""
    torch = pytest.importorskip("torch")
    hip, cpu = scorers("1k4c")
    poses = case_positions("1k4c", orc)[:32]
    dev = torch.device("cuda:0")
    d_poses = torch.from_numpy(poses).to(dev)
    d_out = torch.zeros(32, dtype=torch.float64, device=dev)
    d_cnt = torch.zeros(32, dtype=torch.int32, device=dev)
    hip.energy_batch_device(32, d_poses.data_ptr(), 7, d_out.data_ptr(), None, d_cnt.data_ptr())
    blocks = hip.last_block_counts(32).astype(np.int64)
    hits = d_cnt.cpu().numpy().astype(np.int64)
    all_blocks = 3413 * 3268 / 64.0
    assert np.all(blocks * 64 >= hits)
    assert blocks.mean() < 0.08 * all_blocks          # ~3.7 % of the pair blocks survive the box tests
    dna, _ = scorers("1azp")
    with pytest.raises(pkg.LightdockError, match="tiled DFIRE kernel only"):
        dna.last_block_counts(4)


def test_gso_config5_per_gpu_share(pkg, scorers, orc):
    """BASELINE config 5 as one GPU sees it (1024 swarms over 8 GPUs = 128 swarms x 200
    glowworms, 1ppe DFIRE): size-independent properties at full size -- replicated swarms stay
    bit-identical wherever they sit in the batch, sampled swarms equal the oracle, the
    evaluation count is the number of moved glowworms."""
    hip, cpu = scorers("1ppe")
    base = case_positions("1ppe", orc)
    n_swarms, steps = 128, 8
    swarms = [base] + [pkg.synth.swarm(200, seed=k) for k in range(1, n_swarms)]
    swarms[77] = swarms[3]                     # two replicated pairs
    swarms[127] = swarms[0]
    gso = pkg.GSO(hip, np.stack(swarms))
    gso.run(steps)
    a, b = gso.read(3), gso.read(77)
    c, d = gso.read(0), gso.read(127)
    for k in ("poses", "luciferin", "scoring", "n_neighbors", "target"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(c[k], d[k]), k
    total = 0
    for s in (0, 3, 64):
        ref = orc.GSO(cpu, swarms[s])
        for _ in range(steps):
            ref.step()
        st, want = gso.read(s), ref.state()
        assert np.array_equal(st["n_neighbors"], want["n_neighbors"]) and np.array_equal(st["target"], want["target"])
        assert bm_err(st["scoring"], want["scoring"]) < REL_TOL
        total += ref.num_evals
    assert gso.num_evals >= total and gso.steps_done == steps


def _random_protein_pdb(path, n_atoms, seed, box):
    """A fake but DFIRE-typable molecule: residues cycled from a template list, atoms placed at
    random inside a box (density is irrelevant for parity)."""
    templ = [("ALA", ["N", "CA", "C", "O", "CB"]), ("LEU", ["N", "CA", "C", "O", "CB", "CG", "CD1", "CD2"]),
             ("LYS", ["N", "CA", "C", "O", "CB", "CG", "CD", "CE", "NZ"]), ("GLY", ["N", "CA", "C", "O"]),
             ("TRP", ["N", "CA", "C", "O", "CB", "CG", "CD1", "CD2", "NE1", "CE2", "CE3", "CZ2", "CZ3", "CH2"]),
             ("SER", ["N", "CA", "C", "O", "CB", "OG"]), ("ASP", ["N", "CA", "C", "O", "CB", "CG", "OD1", "OD2"])]
    rng = np.random.default_rng(seed)
    atoms, res = [], 0
    while len(atoms) < n_atoms:
        name, names = templ[res % len(templ)]
        centre = rng.uniform(-box, box, size=3)
        for a in names:
            if len(atoms) == n_atoms:
                break
            p = centre + rng.normal(0, 1.5, size=3)
            atoms.append((a, name, "A", res % 9000 + 1, p[0], p[1], p[2]))
        res += 1
    _write_pdb(path, atoms)


@pytest.mark.parametrize("n_rec,box", [(4700, 30.0), (9000, 38.0), (17000, 47.0), (21000, 50.5), (28500, 56.0)])
def test_receptor_larger_than_one_ballot(pkg, orc, table, tmp_path, n_rec, box):
    """More than 64 receptor tiles (> 4096 atoms: the tile-box ballot loops) and a ligand that is
    not a multiple of 64, against the oracle and the all-pairs kernel.  141 tiles (9000 atoms) also take the culling
    kernel's LDS (receptor boxes + hit lists) past 64 KB, i.e. through hipFuncSetAttribute; 266 tiles (17 000 atoms) are
    past the 255 an entry of the block-major path could name until round 4; 329 tiles (21 000 atoms) leave the culling kernel's
    waves a shorter hit list (its LDS holds every receptor box); 446 tiles (28 500 atoms) do not fit that LDS at all: the
    pose-major kernel takes the complex, silently and with the same numbers."""
    rec, lig = str(tmp_path / "big_rec.pdb"), str(tmp_path / "big_lig.pdb")
    _random_protein_pdb(rec, n_rec, 1, box)
    _random_protein_pdb(lig, 333, 2, 8.0)
    cpu = orc.Scorer("dfire", rec, lig, rec_active=["A.LEU.2", "A.TRP.5"], lig_active=["A.ALA.1"], potential=table)
    hip = pkg.Scorer.from_pdb("dfire", rec, lig, rec_active=["A.LEU.2", "A.TRP.5"], lig_active=["A.ALA.1"], potential=table)
    assert hip.num_atoms(0) == n_rec and hip.num_atoms(1) == 333
    assert hip.kernel_info()["pair_kernel_name"] == ("dfire_bm_pairs" if n_rec < 28000 else "dfire_packed_pairs")
    poses = pkg.synth.swarm(24, seed=9)
    poses[:, :3] *= 0.8
    want = cpu.energy_rows(poses)
    assert bm_err(hip.energy_batch(poses), want) < REL_TOL
    os.environ["LIGHTDOCK_DFIRE_KERNEL"] = "allpairs"
    try:
        ap = pkg.Scorer.from_pdb("dfire", rec, lig, rec_active=["A.LEU.2", "A.TRP.5"], lig_active=["A.ALA.1"], potential=table)
    finally:
        os.environ.pop("LIGHTDOCK_DFIRE_KERNEL")
    assert bm_err(ap.energy_batch(poses), want) < REL_TOL


def test_receptor_too_long_for_the_packed_frame(pkg, orc, table, tmp_path):
    """A receptor more than ~8100 A long on one axis: no f32 frame of the packed kernels holds it with a small enough error
    bound (scorer.cpp, packed_accepts), so the scorer takes the all-pairs kernel -- the oracle's energies and in-cutoff pair
    counts.  Two residue clumps 8300 A apart, the ligand posed next to either of them or far from both."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(41)
    rec, lig = str(tmp_path / "long_rec.pdb"), str(tmp_path / "long_lig.pdb")
    clumps = [_random_molecule(rng, 150, 16.0, "A"), _random_molecule(rng, 150, 16.0, "A")]
    _write_pdb(rec, [(a, r, c, seq + 100 * k, x + x0, y, z) for k, x0 in enumerate((-900.0, 7400.0)) for a, r, c, seq, x, y, z in clumps[k]])
    _write_pdb(lig, _random_molecule(rng, 90, 10.0, "B"))
    hip = pkg.Scorer.from_pdb("dfire", rec, lig, potential=table)
    cpu = orc.Scorer("dfire", rec, lig, potential=table)
    assert hip.kernel_info()["pair_kernel_name"] == "pose_energy_pairs<0"
    q = rng.normal(size=(24, 4))
    t = np.array([-900.0, 0.0, 0.0]) + rng.uniform(-10.0, 10.0, size=(24, 3))
    t[16:22, 0] += 8300.0        # next to the other clump
    t[22:, 0] = 3000.0           # between them: nothing in range
    poses = np.ascontiguousarray(np.concatenate([t, q / np.linalg.norm(q, axis=1, keepdims=True)], axis=1))
    want = [cpu.energy_ex_row(p) for p in poses]
    want_counts = np.array([w[1][5] for w in want]).astype(np.int64)
    assert np.all(want_counts[:22] > 0) and np.all(want_counts[22:] == 0)
    dev = torch.device("cuda:0")
    d_poses = torch.from_numpy(poses).to(dev)
    d_out = torch.zeros(len(poses), dtype=torch.float64, device=dev)
    d_cnt = torch.zeros(len(poses), dtype=torch.int32, device=dev)
    hip.energy_batch_device(len(poses), d_poses.data_ptr(), 7, d_out.data_ptr(), None, d_cnt.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d_cnt.cpu().numpy().astype(np.int64), want_counts)
    assert rel_err(d_out.cpu().numpy(), np.array([w[0] for w in want])) < REL_TOL
    assert rel_err(hip.energy_batch(poses), np.array([w[0] for w in want])) < REL_TOL


def test_which_kernel_a_flexing_complex_gets(pkg, orc, table, tmp_path):
    """The fallbacks of the block-major path's ANM form as a stated contract (VERDICT r05 item 5 ii; lightdock-rust_amd/csrc/scorer.cpp,
    bm_accepts): up to ten modes a molecule run `dfire_bm_pairs` -- since round 6 also with a receptor of 8192 atoms or more (the
    fixed-point scale then allows for the atoms a flexed ligand tile can reach) --, an eleventh mode sends the complex to the
    pose-major `dfire_packed_pairs`; both give the oracle's energies and in-cutoff pair counts (src/dfire.rs:288-320)."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(77)
    rec, lig = str(tmp_path / "flex_rec.pdb"), str(tmp_path / "flex_lig.pdb")
    _random_protein_pdb(rec, 9000, 3, 38.0)
    _random_protein_pdb(lig, 140, 4, 6.0)
    dev = torch.device("cuda:0")
    for n_rec_modes, n_lig_modes, want_kernel in ((3, 10, "dfire_bm_pairs"), (11, 2, "dfire_packed_pairs"), (0, 11, "dfire_packed_pairs")):
        kw = dict(potential=table, use_anm=True, rec_num_anm=n_rec_modes, lig_num_anm=n_lig_modes,
                  rec_nmodes=rng.normal(0.0, 0.02, size=n_rec_modes * 9000 * 3) if n_rec_modes else None,
                  lig_nmodes=rng.normal(0.0, 0.1, size=n_lig_modes * 140 * 3) if n_lig_modes else None)
        hip = pkg.Scorer.from_pdb("dfire", rec, lig, **kw)
        cpu = orc.Scorer("dfire", rec, lig, **kw)
        assert hip.kernel_info()["pair_kernel_name"] == want_kernel, (n_rec_modes, n_lig_modes)
        poses = pkg.synth.swarm(16, seed=21)
        poses[:, :3] *= 0.9
        poses = np.ascontiguousarray(np.concatenate([poses[:, :7], rng.normal(0.0, 3.0, size=(16, n_rec_modes + n_lig_modes))], axis=1))
        want = [cpu.energy_ex_row(p) for p in poses]
        d_poses = torch.from_numpy(poses).to(dev)
        d_out = torch.zeros(len(poses), dtype=torch.float64, device=dev)
        d_cnt = torch.zeros(len(poses), dtype=torch.int32, device=dev)
        hip.energy_batch_device(len(poses), d_poses.data_ptr(), poses.shape[1], d_out.data_ptr(), None, d_cnt.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_cnt.cpu().numpy().astype(np.int64), np.array([w[1][5] for w in want]).astype(np.int64))
        err = bm_err if want_kernel == "dfire_bm_pairs" else rel_err
        assert err(d_out.cpu().numpy(), np.array([w[0] for w in want])) < REL_TOL


def test_bench_plain_command_runs_n_ranks(pkg):
    """`python bench.py --gpus 2` (no torchrun): bench.py starts the two ranks itself; on this 1-GPU box both are pinned to
    device 0 (LD_BENCH_FORCE_DEVICE) and the timing collectives go over gloo.  One JSON line, n_gpus 2, whole-job value."""
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LD_BENCH_FORCE_DEVICE="0")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([os.sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--backend", "gloo", "--workload", "gso-1ppe",
                        "--swarms", "8", "--steps", "3", "--warmup", "1", "--cpu-seconds", "0"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["scaling"] == "strong" and out["value"] > 0
    assert out["config"]["swarms_this_rank"] == 4
    # without the override the same command must refuse rather than share one GPU silently
    env.pop("LD_BENCH_FORCE_DEVICE")
    r = subprocess.run([os.sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--backend", "gloo", "--steps", "1"], env=env,
                       capture_output=True, text=True, timeout=300)
    if pkg.device_count() < 2:
        assert r.returncode != 0 and "device(s) visible" in r.stderr


@pytest.mark.parametrize("name", ["1ppe", "1k4c"])
def test_block_major_frame_edges_and_absurd_poses(pkg, scorers, orc, name):
    """The block-major path keeps f32 records in a frame that holds the receptor + 16 A; a ligand atom outside it is
    beyond the cutoff of every receptor atom and joins no box.  Poses that put the ligand half outside the frame, far
    outside, thousands of angstroms away, on top of the receptor (every pair clashing: the exact-path queue is drained
    over and over) and with a zero or non-finite quaternion must give the oracle's energies and in-cutoff pair counts,
    and must not disturb their neighbours in the batch."""
    torch = pytest.importorskip("torch")
    hip, cpu = scorers(name)
    assert hip.kernel_info()["pair_kernel_name"] == "dfire_bm_pairs"
    base = case_positions(name, orc)[:40].copy()
    rng = np.random.default_rng(3)
    poses = base.copy()
    direction = rng.normal(size=(40, 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    reach = np.array([0, 0, 0, 0, 5, 20, 40, 60, 80, 100, 120, 140, 160, 200, 300, 1e3, 1e4, 1e6, 1e9, 1e15])
    poses[:20, :3] = direction[:20] * reach[:, None]      # from on top of the receptor to absurdly far
    poses[20, 3:7] = 0.0                                   # zero quaternion: NaN coordinates in the reference, no pair in range
    poses[21, 3:7] *= 1e-3                                 # tiny and huge norms: rotate divides by the norm
    poses[22, 3:7] *= 1e3
    want = np.array([cpu.energy_ex_row(p) for p in poses], dtype=object)
    want_e = np.array([w[0] for w in want], dtype=np.float64)
    want_n = np.array([w[1][5] for w in want]).astype(np.int64)
    dev = torch.device("cuda:0")
    d_poses = torch.from_numpy(poses).to(dev)
    d_out = torch.zeros(len(poses), dtype=torch.float64, device=dev)
    d_cnt = torch.zeros(len(poses), dtype=torch.int32, device=dev)
    hip.energy_batch_device(len(poses), d_poses.data_ptr(), poses.shape[1], d_out.data_ptr(), None, d_cnt.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d_cnt.cpu().numpy().astype(np.int64), want_n)
    assert bm_err(d_out.cpu().numpy(), want_e) < REL_TOL
    assert bm_err(hip.energy_batch(poses), want_e) < REL_TOL
    assert want_n[:4].min() > 10000 and np.all(want_n[15:21] == 0)
    assert np.array_equal(hip.energy_batch(poses)[23:], hip.energy_batch(base[23:]))     # the neighbours: bit for bit what they are alone


@pytest.mark.gpu
def test_block_major_anm_form_and_wild_amplitudes(pkg, scorers, orc):
    """DFIRE with normal modes (src/dfire.rs:288-320) runs the block-major path's ANM form: both molecules flex per pose
    inside the batch.  Its f32 bounds cover deformations up to 16 A per coordinate (round 6; 32 A before); a pose whose amplitudes
    could exceed that (|amplitudes|_2 x the largest 2-norm of an atom's mode components, Cauchy-Schwarz) -- or are not
    finite -- is WILD: every block of it goes to the exact path.  Ordinary, large, absurd, NaN and infinite amplitudes must
    give the oracle's energies and in-cutoff pair counts, and leave their neighbours bit for bit what they are alone."""
    torch = pytest.importorskip("torch")
    hip, cpu = scorers("2uuy")
    assert hip.kernel_info()["pair_kernel_name"] == "dfire_bm_pairs"
    base = case_positions("2uuy", orc)[:32].copy()
    poses = base.copy()
    assert poses.shape[1] == 27
    scale = [1, 2, 5, 10, 20, 50, 100, 300, 1e3, 1e5]
    for i, f in enumerate(scale):
        poses[i, 7:] *= f
    poses[10, 7:17] *= 40.0        # the receptor alone flexes wildly
    poses[11, 17:] *= 40.0         # the ligand alone
    poses[12, 9] = np.nan
    poses[13, 20] = np.inf
    poses[14, 7:] = 0.0            # a rigid pose among them
    poses[15, 7] = 1e300
    want = [cpu.energy_ex_row(p) for p in poses]
    want_e = np.array([w[0] for w in want], dtype=np.float64)
    want_n = np.array([w[1][5] for w in want]).astype(np.int64)
    dev = torch.device("cuda:0")
    d_poses = torch.from_numpy(poses).to(dev)
    d_out = torch.zeros(len(poses), dtype=torch.float64, device=dev)
    d_cnt = torch.zeros(len(poses), dtype=torch.int32, device=dev)
    hip.energy_batch_device(len(poses), d_poses.data_ptr(), poses.shape[1], d_out.data_ptr(), None, d_cnt.data_ptr())
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert np.array_equal(d_cnt.cpu().numpy().astype(np.int64), want_n)
    finite = np.isfinite(want_e)
    assert np.array_equal(np.isnan(got), np.isnan(want_e))
    assert bm_err(got[finite], want_e[finite]) < REL_TOL
    again = hip.energy_batch(poses)
    assert bm_err(again[finite], want_e[finite]) < REL_TOL
    assert np.array_equal(again[16:], hip.energy_batch(base[16:]))


@pytest.mark.gpu
@pytest.mark.parametrize("n_rec_modes,n_lig_modes", [(10, 0), (0, 10), (3, 7), (1, 1)])
def test_block_major_anm_with_one_rigid_molecule_or_fewer_modes(pkg, orc, table, n_rec_modes, n_lig_modes):
    """The ANM form keeps room for ten modes a molecule; fewer (or none on one side: src/dfire.rs:288-320 loops over what the
    model holds) leave amplitudes and modes zero there.  Energies and in-cutoff pair counts against the oracle built the same way."""
    torch = pytest.importorskip("torch")
    method, rec, lig, kw = case_kwargs("2uuy", orc, table)
    full_rec, full_lig = np.asarray(kw["rec_nmodes"], dtype=np.float64).ravel(), np.asarray(kw["lig_nmodes"], dtype=np.float64).ravel()
    kw = dict(kw, rec_num_anm=n_rec_modes, lig_num_anm=n_lig_modes,
              rec_nmodes=full_rec[: full_rec.size // 10 * n_rec_modes] if n_rec_modes else None,
              lig_nmodes=full_lig[: full_lig.size // 10 * n_lig_modes] if n_lig_modes else None)
    hip = pkg.Scorer.from_pdb(method, rec, lig, **kw)
    cpu = orc.Scorer(method, rec, lig, **kw)
    assert hip.kernel_info()["pair_kernel_name"] == "dfire_bm_pairs"
    base = case_positions("2uuy", orc)[:48]
    poses = np.ascontiguousarray(np.concatenate([base[:, :7], base[:, 7:7 + n_rec_modes], base[:, 17:17 + n_lig_modes]], axis=1))
    want = [cpu.energy_ex_row(p) for p in poses]
    want_e = np.array([w[0] for w in want], dtype=np.float64)
    want_n = np.array([w[1][5] for w in want]).astype(np.int64)
    dev = torch.device("cuda:0")
    d_poses = torch.from_numpy(poses).to(dev)
    d_out = torch.zeros(len(poses), dtype=torch.float64, device=dev)
    d_cnt = torch.zeros(len(poses), dtype=torch.int32, device=dev)
    hip.energy_batch_device(len(poses), d_poses.data_ptr(), poses.shape[1], d_out.data_ptr(), None, d_cnt.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d_cnt.cpu().numpy().astype(np.int64), want_n)
    assert bm_err(d_out.cpu().numpy(), want_e) < REL_TOL


def _counts_of(torch, scorer, poses):
    dev = torch.device("cuda:0")
    d_poses = torch.from_numpy(np.ascontiguousarray(poses)).to(dev)
    d_out = torch.zeros(len(poses), dtype=torch.float64, device=dev)
    d_cnt = torch.zeros(len(poses), dtype=torch.int32, device=dev)
    scorer.energy_batch_device(len(poses), d_poses.data_ptr(), poses.shape[1], d_out.data_ptr(), None, d_cnt.data_ptr())
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_cnt.cpu().numpy()


@pytest.mark.gpu
def test_membrane_beads_with_zero_rows_are_listed_within_the_interface_distance_only(pkg, orc, table):
    """VERDICT r05 item 8.  A receptor type whose rows of the potential are 0.0 against every ligand type of the complex adds
    nothing at any distance (src/dfire.rs:338): the culling kernel lists the blocks of a subtile of such atoms -- 1k4c's membrane
    beads, type 167, if the DCparams at hand has zero rows for them -- within the interface distance only (src/dfire.rs:339:
    the beads' interface flags are what the membrane penalty counts, src/dfire.rs:355-359).  Energies, membrane terms and
    in-cutoff pair counts must stay the oracle's with the same table; a table with ONE nonzero value in those rows has no
    such subtile."""
    torch = pytest.importorskip("torch")
    t = table.copy()
    t.reshape(169, 169, 20)[167, :, :] = 0.0
    method, rec, lig, kw = case_kwargs("1k4c", orc, t)
    hip, cpu = pkg.Scorer.from_pdb(method, rec, lig, **kw), orc.Scorer(method, rec, lig, **kw)
    assert hip.kernel_info()["pair_kernel_name"] == "dfire_bm_pairs"
    quiet = hip.bm_quiet_subtiles()
    assert 38 <= quiet <= 60, quiet          # 453 beads: 38 subtiles of beads only in the library's order (+ a few after re-ordering)
    poses = case_positions("1k4c", orc)
    want = cpu.energy_rows(poses)
    stats = np.array([cpu.energy_ex_row(p)[1] for p in poses[:60]])
    assert (stats[:, 4] > 0).sum() >= 3, "membrane-intersecting poses: the beads' interface flags must still be found"
    assert bm_err(hip.energy_batch(poses), want) < REL_TOL
    got, counts = _counts_of(torch, hip, poses[:60])
    assert bm_err(got, want[:60]) < REL_TOL
    assert np.array_equal(counts.astype(np.int64), stats[:, 5].astype(np.int64))      # a counting launch counts every pair inside the cutoff
    # the same poses pushed into the membrane: many beads within 2.45 A of ligand atoms
    deep = poses[:40].copy()
    deep[:, 2] += np.linspace(-25.0, 25.0, 40)
    assert bm_err(hip.energy_batch(deep), cpu.energy_rows(deep)) < REL_TOL
    # one nonzero value in the beads' rows -- in the read PAST the row of the last ligand type present, at r = 15.0 exactly
    # (bin 20 = the next type's bin 0, src/dfire.rs:336-338) -- and no subtile is quiet any more
    lig_types = np.unique(cpu.model(1)["dfire_types"])
    t2 = t.copy()
    t2.reshape(-1)[167 * 169 * 20 + int(lig_types[-1]) * 20 + 20] = 1.5
    method, rec, lig, kw = case_kwargs("1k4c", orc, t2)
    assert pkg.Scorer.from_pdb(method, rec, lig, **kw).bm_quiet_subtiles() == 0
    method, rec, lig, kw = case_kwargs("1k4c", orc, table)
    assert pkg.Scorer.from_pdb(method, rec, lig, **kw).bm_quiet_subtiles() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("restraints,modes", [(False, 0), (True, 0), (True, 6)])
def test_receptor_types_with_zero_rows_in_random_molecules(pkg, orc, table, tmp_path, restraints, modes):
    """Random molecules, the rows of most receptor types zeroed: subtiles of such atoms only are never listed when no atom of
    the complex has an interface-flag slot, within 2.45 A when one has (a ligand restraint's flag can be set by ANY receptor
    atom, src/dfire.rs:339-342) -- rigid form and ANM form (the reach travels with the flexed receptor's boxes)."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(77 + modes)
    rec, lig = str(tmp_path / "rec.pdb"), str(tmp_path / "lig.pdb")
    rec_atoms = _random_molecule(rng, 1100, 30.0, "A")
    lig_atoms = _random_molecule(rng, 300, 18.0, "B")
    _write_pdb(rec, rec_atoms)
    _write_pdb(lig, lig_atoms)
    kw = {}
    if restraints:
        kw = dict(rec_active=["A.%s.%d" % (rec_atoms[0][1], rec_atoms[0][3])], lig_active=["B.%s.%d" % (lig_atoms[-1][1], lig_atoms[-1][3])])
    n_poses, cols = 32, 7 + 2 * modes
    if modes:
        kw.update(use_anm=True, rec_num_anm=modes, lig_num_anm=modes,
                  rec_nmodes=(rng.normal(size=(modes, 1100, 3)) * 0.4).ravel(), lig_nmodes=(rng.normal(size=(modes, 300, 3)) * 0.4).ravel())
    probe = orc.Scorer("dfire", rec, lig, potential=table, **kw)
    rec_types = np.unique(probe.model(0)["dfire_types"])
    silent = rng.permutation(rec_types)[: int(0.93 * len(rec_types))]
    t = table.copy()
    t.reshape(169, 169, 20)[silent, :, :] = 0.0
    cpu = orc.Scorer("dfire", rec, lig, potential=t, **kw)
    hip = pkg.Scorer.from_pdb("dfire", rec, lig, potential=t, **kw)
    assert hip.kernel_info()["pair_kernel_name"] == "dfire_bm_pairs"
    assert hip.bm_quiet_subtiles() >= 20, hip.bm_quiet_subtiles()
    poses = np.zeros((n_poses, cols))
    poses[:, :3] = rng.uniform(-22, 22, (n_poses, 3))
    poses[:6, :3] = rng.uniform(-2, 2, (6, 3))                 # overlapping: clashes, interface flags
    q = rng.normal(size=(n_poses, 4))
    poses[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    if modes:
        poses[:, 7:] = rng.normal(size=(n_poses, 2 * modes)) * 2.0
        poses[::10, 7:] *= 40.0                                  # wild poses: every block of every tile pair, through the exact path
    want = cpu.energy_rows(poses)
    if restraints:
        stats = np.array([cpu.energy_ex_row(p)[1] for p in poses[:6]])
        assert (stats[:, 2] + stats[:, 3] > 0).any(), "an overlapping pose should satisfy a restraint"
    assert bm_err(hip.energy_batch(poses), want) < REL_TOL
    got, counts = _counts_of(torch, hip, poses)
    assert bm_err(got, want) < REL_TOL
    assert np.array_equal(counts[:8].astype(np.int64), np.array([cpu.energy_ex_row(p)[1][5] for p in poses[:8]]).astype(np.int64))
