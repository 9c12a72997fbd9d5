"""Local refinement on the GPU (include/lightdock_hip.h "Local refinement") against its numpy restatement
(tests/refine_reference.py):

  1. ld_refine_trials equals the restatement's bits: shapes past one wave, past two and at the largest pose, strided rows,
     per-pose steps after 0-5 halvings, frozen poses, non-unit / zero / NaN quaternions and NaN coordinates;
  2. ld_refine_select equals the restatement's bits on injected energies: NaN, +-inf, all-NaN rows, equal maxima in different
     lanes and in one lane's stride, a maximum equal to E, halvings at the limit, garbage in frozen poses' rows;
  3. the device loop equals the same loop driven from the host through ld_refine_trials, energy_batch and ld_refine_select,
     to the bit (precondition, asserted on its own: energy_batch gives the same bits twice);
  4. the device loop equals the restatement driven by the CPU oracle for every row of refine_cases.TABLE: history and
     poses to the bit (pose arithmetic never sees an energy; every decision gap of the oracle is above 1e-5, so no pose is
     left out), energies within the fixture's measure;
  5. properties on 1ppe: energies, monotonicity, slices, refusals, n == 0, and a GSO that goes on to the same bits after a
     refinement grew the scorer's workspace;
  6. the tool on a small 1czy run.

The energies' measures are those of tests/test_gpu_parity.py (copied, not imported): REL_TOL = 1e-9 relative, `bm_err` where
the block-major DFIRE path runs (an absolute allowance of 1e-11 for its fixed-point sums).
"""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, case_kwargs, case_positions
import refine_reference as rr
from refine_cases import MIN_GAP, TABLE, TABLE_IDS, oracle_refinement, tool_module

pytestmark = pytest.mark.gpu

REL_TOL = 1e-9
BM_ATOL = 1e-11


def rel_err(got, want):
    return np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-9))


def bm_err(got, want):
    return np.max(np.maximum(np.abs(got - want) - BM_ATOL, 0.0) / np.maximum(np.abs(want), 1e-9))


def err_of(hip):
    return bm_err if hip.kernel_info()["pair_kernel_name"] == "dfire_bm_pairs" else rel_err


def same_bits(a, b):
    """Equal to the bit, a NaN matching any NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan])


def same_state(a, b):
    return all(same_bits(a[k], b[k]) if a[k].dtype == np.float64 else np.array_equal(a[k], b[k]) for k in a)


@pytest.fixture(scope="module")
def scorers(pkg, orc, table):
    pkg.init(0)
    cache = {}

    def get(name, method=None):
        if (name, method) not in cache:
            own, rec, lig, kw = case_kwargs(name, orc, table)
            cache[(name, method)] = pkg.Scorer.from_pdb(method or own, rec, lig, **kw)
        return cache[(name, method)]
    return get


SHAPES_N = (1, 63, 65, 257)
POSE_LENS = (7, 8, 27, 73, 135)


def random_case(rng, n, pose_len, stride):
    """Poses with the awkward rows, and a state with per-pose steps after 0-5 halvings and random frozen bytes."""
    poses = rng.standard_normal((n, stride)) * 5.0
    poses[:, 3:7] /= np.linalg.norm(poses[:, 3:7], axis=1)[:, None]
    for p in range(n):
        kind = p % 8
        if kind == 1:
            poses[p, 3:7] *= 1.7                      # not a unit quaternion
        elif kind == 2:
            poses[p, 3:7] = 0.0
        elif kind == 3:
            poses[p, 3 + p % 4] = np.nan
        elif kind == 4:
            poses[p, p % 3] = np.nan
        elif kind == 5 and pose_len > 7:
            poses[p, 7 + p % (pose_len - 7)] = np.nan
        elif kind == 6:
            poses[p, 3:7] = [0.0, -0.0, 1.0, -0.0]    # signed zeros through the product
    state = rr.start_state(rng.standard_normal(n), 1.0 + rng.random(), 0.1 + rng.random(), 0.5 + rng.random())
    for p in range(n):
        for _ in range(int(rng.integers(0, 6))):
            rr.halve(state, p)
    state["frozen"][:] = rng.random(n) < 0.3
    state["accepted"][:] = rng.integers(0, 9, n)
    state["evaluations"][:] = rng.integers(1, 999, n)
    return poses, state


@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("pose_len", POSE_LENS)
def test_trials_equal_the_restatement(pkg, orc, pose_len, extra):
    pkg.init(0)
    K, stride = rr.trial_count(pose_len), pose_len + extra
    rng = np.random.default_rng(1000 * pose_len + extra)
    for n in SHAPES_N:
        poses, state = random_case(rng, n, pose_len, stride)
        before = rr.copy_state(state)
        sentinel = rng.standard_normal((n, K, stride))
        got, active = pkg.refine_trials(poses, pose_len, state, sentinel, active=np.full((n, K), 7, dtype=np.uint8))
        want, want_active = rr.trials(orc.q_mul, poses, pose_len, state)
        live = state["frozen"] == 0
        assert np.array_equal(active, want_active), (n, pose_len)
        assert same_bits(got[live][:, :, :pose_len], want[live]), (n, pose_len)
        assert same_bits(got[~live], sentinel[~live])                          # a frozen pose's rows are untouched
        assert same_bits(got[:, :, pose_len:], sentinel[:, :, pose_len:])      # and so is everything beyond pose_len
        assert same_state(state, before)


def injected_energies(rng, n, K, state, max_halvings):
    e = rng.standard_normal((n, K))
    for p in range(n):
        kind = p % 12
        E = state["energy"][p]
        j1 = int(rng.integers(0, K))
        if kind == 1:
            e[p, rng.random(K) < 0.4] = np.nan
        elif kind == 2:
            e[p, j1] = np.inf
        elif kind == 3:
            e[p] = -np.inf
        elif kind == 4:
            e[p] = np.nan
        elif kind in (5, 6):                          # equal maxima at two j: in different lanes / in one lane's stride
            d = 64 if kind == 6 and K > 64 else 1 + int(rng.integers(0, min(K, 64) - 1))
            j1 = int(rng.integers(0, K - d))
            j2 = j1 + d
            assert j2 < K and ((j2 - j1) % 64 == 0) == (kind == 6 and K > 64)
            e[p, [j1, j2]] = max(np.nanmax(e[p]), E) + 1.0
        elif kind == 7:                               # the maximum equals E: no accept
            e[p] = np.minimum(e[p], E)
            e[p, j1] = E
        elif kind == 8:                               # a failure at the limit: the pose freezes
            e[p] = E - 1.0 - rng.random(K)
            state["halvings"][p] = max_halvings
        elif kind == 9:
            state["energy"][p] = np.nan
        elif kind == 10:
            e[p, j1] = -np.inf
            e[p, (j1 + 1) % K] = np.nan
        if state["frozen"][p]:                        # garbage the kernel must not read
            e[p] = np.where(rng.random(K) < 0.5, np.nan, 1e300)
    return e


@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("pose_len", POSE_LENS)
def test_select_equals_the_restatement_on_injected_energies(pkg, orc, pose_len, extra):
    pkg.init(0)
    K, stride, max_halvings = rr.trial_count(pose_len), pose_len + extra, 3
    rng = np.random.default_rng(2000 * pose_len + extra)
    seen = set()
    for n in SHAPES_N:
        poses, state = random_case(rng, n, pose_len, stride)
        energies = injected_energies(rng, n, K, state, max_halvings)
        got_poses, got_state, got_history = pkg.refine_select(poses, pose_len, state, energies, max_halvings)
        want_poses, want_state = poses.copy(), rr.copy_state(state)
        want_history = rr.select(orc.q_mul, want_poses, pose_len, want_state, energies, max_halvings)
        assert np.array_equal(got_history, want_history), (n, pose_len)
        assert same_bits(got_poses, want_poses), (n, pose_len)
        assert same_state(got_state, want_state), (n, pose_len)
        frozen = state["frozen"] == 1
        assert np.all(got_history[frozen] == rr.NOT_EVALUATED) and same_bits(got_poses[frozen], poses[frozen])
        for p in np.flatnonzero(~frozen):
            if p % 12 in (5, 6):                      # of two equal maxima the lower index wins
                top = np.flatnonzero(energies[p] == np.nanmax(energies[p]))
                assert len(top) == 2 and got_history[p] == top[0]
            if p % 12 in (3, 4, 7, 8):
                assert got_history[p] < 0 and same_bits(got_poses[p], poses[p])
        seen |= set(got_history.tolist())
    assert {rr.HALVED, rr.FROZEN, rr.NOT_EVALUATED} <= seen and max(seen) >= K // 2    # every outcome, moves of every kind


# ---------------------------------------------------------------------------------------------------------------------
# 3. the device loop against the host-driven loop
# ---------------------------------------------------------------------------------------------------------------------
def host_driven(pkg, hip, poses, iterations, max_halvings, steps):
    """What a user has without ld_scorer_refine: the two kernels' entry points and energy_batch on the n x K rows."""
    pose_len = hip.pose_len
    n, K = poses.shape[0], rr.trial_count(pose_len)
    poses = np.array(poses[:, :pose_len])
    before = hip.energy_batch(poses)
    state = rr.start_state(before, *steps)
    trials = np.zeros((n, K, pose_len))
    history = np.zeros((n, iterations), dtype=np.int16)
    for it in range(iterations):
        trials, _ = pkg.refine_trials(poses, pose_len, state, trials)
        energies = hip.energy_batch(trials.reshape(n * K, pose_len)).reshape(n, K)
        poses, state, history[:, it] = pkg.refine_select(poses, pose_len, state, energies, max_halvings)
    return poses, before, state, history


LOOP_ROWS = [r for r in TABLE if r[1] is None and r[0] in ("1ppe", "2uuy", "1azp")]


@pytest.mark.parametrize("row", LOOP_ROWS, ids=[i for r, i in zip(TABLE, TABLE_IDS) if r in LOOP_ROWS])
def test_energy_batch_gives_the_same_bits_twice(scorers, orc, row):
    """The precondition of the comparison below, on its own."""
    hip = scorers(row[0])
    poses = np.ascontiguousarray(case_positions(row[0], orc)[:row[2]])
    assert same_bits(hip.energy_batch(poses), hip.energy_batch(poses))


@pytest.mark.parametrize("row", LOOP_ROWS, ids=[i for r, i in zip(TABLE, TABLE_IDS) if r in LOOP_ROWS])
def test_loop_equals_the_host_driven_loop(pkg, scorers, orc, row):
    name, _, n, iterations, steps, max_halvings = row[:6]
    hip = scorers(name)
    poses = np.ascontiguousarray(case_positions(name, orc)[:n])
    assert same_bits(hip.energy_batch(poses), hip.energy_batch(poses))
    got = hip.refine(poses, iterations, *steps, max_halvings=max_halvings, history=True)
    want_poses, want_before, want_state, want_history = host_driven(pkg, hip, poses, iterations, max_halvings, steps)
    assert np.array_equal(got["history"], want_history)
    assert same_bits(got["poses"], want_poses)
    st = got["stats"]
    assert same_bits(st["energy_before"], want_before) and same_bits(st["energy_after"], want_state["energy"])
    for k in ("accepted", "halvings", "evaluations", "frozen"):
        assert np.array_equal(st[k], want_state[k]), k
    info = hip.refine_info()
    assert info["trials"] == rr.trial_count(hip.pose_len) and info["evaluations"] == int(st["evaluations"].sum())
    assert info["last_kernel_ms"] > 0.0 and info["slice"] == 65536 // info["trials"]


# ---------------------------------------------------------------------------------------------------------------------
# 4. the device loop against the restatement driven by the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", TABLE, ids=TABLE_IDS)
def test_loop_equals_the_restatement_driven_by_the_oracle(scorers, orc, table, row):
    name, method, n, iterations, steps, max_halvings = row[:6]
    poses, want = oracle_refinement(orc, table, row)
    assert want["min_gap"] > MIN_GAP                  # so no pose is left out
    hip = scorers(name, method)
    got = hip.refine(poses, iterations, *steps, max_halvings=max_halvings, history=True)
    assert np.array_equal(got["history"], want["history"])
    assert same_bits(got["poses"], want["poses"])
    st, ws = got["stats"], want["state"]
    for k in ("accepted", "halvings", "evaluations", "frozen"):
        assert np.array_equal(st[k], ws[k]), k
    err = err_of(hip)
    figures = (err(st["energy_before"], want["before"]), err(st["energy_after"], want["after"]))
    print("%s: energy error before %.3g after %.3g" % ((name,) + figures))
    assert figures[0] < REL_TOL and figures[1] < REL_TOL


# ---------------------------------------------------------------------------------------------------------------------
# 5. properties on 1ppe
# ---------------------------------------------------------------------------------------------------------------------
def test_properties_on_1ppe(pkg, scorers, orc):
    hip = scorers("1ppe")
    base = np.ascontiguousarray(case_positions("1ppe", orc)[:40])
    poses = np.hstack([base, np.full((40, 2), 7.5)])                          # a stride beyond the pose
    poses[5, 3:7] = 0.0                                                       # a zero quaternion: no trial can be better (every
    got = hip.refine(poses, 8, 1.0, 0.1, 0.5, max_halvings=2, history=True)   # energy NaN, or the same where the ligand is a point)
    st, out = got["stats"], got["poses"]
    assert same_bits(out[5], poses[5, :7]) and same_bits(st["energy_after"][5:6], st["energy_before"][5:6])
    assert st["accepted"][5] == 0 and st["frozen"][5] == 1 and list(got["history"][5]) == [-1, -1, -2] + [-3] * 5
    assert st["halvings"][5] == 2 and st["evaluations"][5] == 1 + 3 * 12
    ok = np.arange(40) != 5
    assert err_of(hip)(st["energy_after"][ok], hip.energy_batch(out[ok])) < REL_TOL
    assert np.all(st["energy_after"][ok] >= st["energy_before"][ok])
    assert np.all((st["energy_after"] > st["energy_before"])[ok] == (st["accepted"] > 0)[ok])
    assert st["accepted"].sum() > 40                                          # the search does move these poses
    tiny = hip.refine(poses, 3, 1e-9, 1e-9, 1e-9, max_halvings=0)             # steps at which many poses gain nothing
    for r in (got, tiny):
        quiet = r["stats"]["accepted"] == 0
        assert quiet[5] and same_bits(r["poses"][quiet], poses[quiet, :7])    # accepted == 0: the pose's own bits

    sliced = hip.refine(poses, 8, 1.0, 0.1, 0.5, max_halvings=2, slice_poses=5, history=True)
    assert hip.refine_info()["slice"] == 5
    assert np.array_equal(sliced["history"], got["history"]) and same_bits(sliced["poses"], out)

    # refusals: LD_ERR_INVALID and every output as it was
    lib = pkg.load_library()
    few = np.ascontiguousarray(poses[:4])
    outs = (np.full((4, 7), -7.5), np.zeros(4, dtype=pkg.REFINE_STATS), np.full((4, 8), 77, dtype=np.int16))
    outs[1].view(np.uint8)[:] = 3
    kept = [a.copy() for a in outs]

    def call(n, stride, iterations=8, trans=1.0, rot=0.1, nm=0.5, slice_poses=0, null_poses=False):
        opts = pkg._RefineOptions(iterations, 2, trans, rot, nm, slice_poses, 0)
        return lib.ld_scorer_refine(hip.handle, C.byref(opts), n, None if null_poses else few.ctypes.data_as(C.c_void_p), stride,
                                    *[a.ctypes.data_as(C.c_void_p) for a in outs])

    for kw in (dict(n=4, stride=9, iterations=0), dict(n=4, stride=9, trans=0.0), dict(n=4, stride=9, trans=-1.0),
               dict(n=4, stride=9, rot=float("nan")), dict(n=4, stride=9, nm=float("inf")), dict(n=4, stride=9, rot=3.1415927),
               dict(n=4, stride=6), dict(n=4, stride=9, null_poses=True), dict(n=2 ** 63, stride=9),
               dict(n=2 ** 64 // 56 + 1, stride=7), dict(n=4, stride=9, slice_poses=(1 << 22) // 12 + 1)):
        assert call(**kw) == -1, kw
        assert lib.ld_last_error()
        assert all(np.array_equal(a, b) for a, b in zip(outs, kept)), kw
    assert call(n=0, stride=9) == 0 and all(np.array_equal(a, b) for a, b in zip(outs, kept))   # n == 0 touches nothing
    assert call(n=4, stride=9) == 0 and same_bits(outs[0], out[:4]) and np.array_equal(outs[2], got["history"][:4])
    assert call(n=4, stride=9, rot=float(np.pi)) == 0                                        # pi itself is allowed


def test_a_gso_goes_on_after_a_refinement_grew_the_workspace(pkg, orc, table):
    """2 steps, a refinement of 300 poses (3600 trial rows through the scorer: its workspace grows and the GSO's graph is
    captured again), 2 more steps: the swarm's state equals an uninterrupted 4-step GSO's to the bit."""
    pkg.init(0)
    method, rec, lig, kw = case_kwargs("1ppe", orc, table)
    pos = np.ascontiguousarray(case_positions("1ppe", orc))
    rng = np.random.default_rng(9)
    many = np.tile(pos, (300 // len(pos) + 1, 1))[:300].copy()
    many[:, :3] += rng.standard_normal((300, 3))
    states = []
    for interrupted in (False, True):
        hip = pkg.Scorer.from_pdb(method, rec, lig, **kw)
        gso = pkg.GSO(hip, pos)
        gso.run(2)
        if interrupted:
            generation_grew = hip.refine(many, 3, 1.0, 0.1, 0.5, max_halvings=1)
            assert generation_grew["stats"]["evaluations"].sum() > 300
        gso.run(2)
        states.append(gso.read(0))
    a, b = states
    assert set(a) == set(b)
    for k in a:
        assert same_bits(a[k], b[k]) if a[k].dtype == np.float64 else np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# 6. the tool
# ---------------------------------------------------------------------------------------------------------------------
def test_refine_tool_on_a_small_1czy_run(pkg, orc, table, tmp_path):
    """The 2-swarm, 10-step DFIRE run of 1czy with the synthetic table that the decomposition tool's test builds; refine.py
    --all --top 12 --pdb 2 on it: the list parses, After >= Before on every row, the rewritten gso files give poses whose
    energy_batch is the listed After, both PDB files hold the complex's atoms."""
    czy = os.path.join(GOLDEN, "1czy")
    run = tmp_path / "run"
    os.makedirs(run / "data")
    for f in ("setup.json", "lightdock_1czy_protein.pdb", "lightdock_1czy_peptide.pdb", "rec_nm.npy", "lig_nm.npy"):
        shutil.copy(os.path.join(czy, f), run)
    pkg.synth.write_dcparams(str(run / "data" / "DCparams"), table)
    pkg.init(0)
    kw = dict(rec_active=["A.SER.467"], use_anm=True, rec_num_anm=10, lig_num_anm=10, rec_nmodes=orc.read_npy(os.path.join(czy, "rec_nm.npy")),
              lig_nmodes=orc.read_npy(os.path.join(czy, "lig_nm.npy")), potential=pkg.load_dcparams(str(run / "data" / "DCparams")))
    hip = pkg.Scorer.from_pdb("dfire", str(run / "lightdock_1czy_protein.pdb"), str(run / "lightdock_1czy_peptide.pdb"), **kw)
    pos = np.stack([orc.parse_positions(os.path.join(czy, "init", "initial_positions_%d.dat" % s)) for s in (0, 1)])
    gso = pkg.GSO(hip, pos, seeds=[324324, 324324])
    gso.run(10)
    for s in (0, 1):
        os.makedirs(run / ("swarm_%d" % s))
    gso.save_many([0, 1], 10, [str(run / "swarm_0"), str(run / "swarm_1")])

    script = os.path.join(os.path.dirname(pkg.__file__), "refine.py")
    r = subprocess.run([sys.executable, script, "setup.json", "10", "dfire", "--swarms", "0-1", "--all", "--top", "12", "--pdb", "2"], cwd=run,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "12 models refined" in r.stdout

    tool, run_dir = tool_module("refine"), tool_module("run_dir")
    head, rows = tool.parse_list((run / "refined" / "refined.list").read_text())
    assert head == tool.REFINED_HEADER.split() and len(rows) == 12 and all(len(x) == len(head) for x in rows)
    col = {h: k for k, h in enumerate(head)}
    after = np.array([float(x[col["After"]]) for x in rows])
    before = np.array([float(x[col["Before"]]) for x in rows])
    assert np.all(after >= before) and list(after) == sorted(after, reverse=True)
    assert any(int(x[col["Accepted"]]) > 0 for x in rows)
    refined = {s: run_dir.read_gso(str(run / "refined" / ("swarm_%d" % s) / "gso_10.out")) for s in (0, 1)}
    original = {s: run_dir.read_gso(str(run / ("swarm_%d" % s) / "gso_10.out")) for s in (0, 1)}
    picked = {(int(x[0]), int(x[1])) for x in rows}
    err = err_of(hip)
    for x, a in zip(rows, after):
        s, g = int(x[0]), int(x[1])
        assert refined[s][1]["scoring"][g] == a
        want = hip.energy_batch(refined[s][0][g][None, :hip.pose_len])[0]
        assert err(np.array([a]), np.array([want])) < REL_TOL
        assert abs(float(x[col["Scoring"]]) - original[s][1]["scoring"][g]) < 1e-5
    for s in (0, 1):                                   # the other glowworms keep their rows
        for g in range(len(original[s][0])):
            if (s, g) not in picked:
                assert np.array_equal(refined[s][0][g], original[s][0][g]) and refined[s][1]["scoring"][g] == original[s][1]["scoring"][g]
        for k in ("rec_id", "lig_id", "luciferin", "neighbors", "vision_range"):
            assert np.array_equal(refined[s][1][k], original[s][1][k])
    atoms = sum(line.startswith(("ATOM", "HETATM")) for f in ("lightdock_1czy_protein.pdb", "lightdock_1czy_peptide.pdb")
                for line in open(run / f))
    for k in (1, 2):
        text = (run / "refined" / ("top_%d.pdb" % k)).read_text()
        assert sum(line.startswith(("ATOM", "HETATM")) for line in text.splitlines()) == atoms
    assert not (run / "refined" / "top_3.pdb").exists()
