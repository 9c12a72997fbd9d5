"""GPU tests of dfire_bm_pairs' exact-path drains (run with -m gpu on an MI355X).

A wave lists the pairs that fall into flagged cells (and, through bm_recheck, those of the blocks with several of them) and
evaluates the list between two jobs, at ONE site of the job loop: trips of four pairs a lane, once more behind the last job
for what is left.  These cases make the lists long and ragged.  COPIES of one pose put the same flagged pair into every lane
of a block's batches, so that a job pushes hundreds to thousands of items: drains of one trip, of several trips with a ragged
last one, the drain behind the last job alone (one pose), and, from the blocks with several flagged pairs, 64 and more
(entry, block) items through bm_recheck and its way back to the drain site when the list of pairs runs out of room.
LIGHTDOCK_BM_PART_CAP=64 makes the jobs short, so that the drains fall on almost every job's end; the ANM form's wild poses
send every pair of theirs to the exact path; every launch here also asks for the pair counts, i.e. runs the same code in
count_mode first.

The copied pose comes from the fixture's first 200 example poses: for 1k4c and 2uuy the one with the most pairs inside the
cutoff (the CPU oracle's count: poses 156 and 79, 270 000 and 76 000 pairs); for 1ppe, whose jobs are short (parts of 128
entries at 300 copies) and whose poses flag fewer than a hundred pairs each, pose 107, one of the two whose flagged pairs
lie close enough together that 300 copies give a drain of three trips even with jobs of 64 entries.  The test itself holds
that the pose has pairs on either side of a bin step: its oracle energy changes when the table's values of one bin are shifted.

Energies are held to the oracle's by the block-major path's error model (bm_err), the in-cutoff pair counts to equality.
The oracle does not say how many pairs its loop would flag, so of the LIGHTDOCK_BM_DEBUG record (columns 20-23: drains, trips,
pairs evaluated, the longest drain's trips) the tests hold that pairs were evaluated at all, that two calls evaluate the
same number, and that the rigid batches of 300 and 1024 copies, and the ANM batch with the wild poses, have a drain of
three trips or more.
"""
import numpy as np
import pytest

from conftest import case_kwargs, case_positions

pytestmark = pytest.mark.gpu

REL_TOL = 1e-9
BM_ATOL = 1e-11
COPIED = {"1k4c": (156, 163), "1ppe": (107, 38), "2uuy": (79, 85)}   # the copied pose, and the one among 255 copies of it
W_DRAINS, W_TRIPS, W_PAIRS, W_MAX_TRIPS = 20, 21, 22, 23


def bm_err(got, want):
    """The block-major path's error model (tests/test_gpu_parity.py): relative error of what exceeds BM_ATOL."""
    return np.max(np.maximum(np.abs(got - want) - BM_ATOL, 0.0) / np.maximum(np.abs(want), 1e-9))


def _debug_record(monkeypatch, tmp_path, hip, poses):
    """One more call with LIGHTDOCK_BM_DEBUG set: the per-wave records of dfire_bm_pairs."""
    path = str(tmp_path / "bm_debug.txt")
    monkeypatch.setenv("LIGHTDOCK_BM_DEBUG", path)
    try:
        hip.energy_batch(np.ascontiguousarray(poses))
    finally:
        monkeypatch.delenv("LIGHTDOCK_BM_DEBUG")
    return np.atleast_2d(np.loadtxt(path))


def _energies_and_counts(hip, poses):
    """A counting launch: the pass in count_mode, then the energies' pass."""
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
def drain_case(pkg, orc, table):
    """Scorers of a fixture and the oracle's energies and pair counts of its poses, computed once per pose.  The copied pose
    has pairs on either side of a bin step: shifting one bin's table values changes its energy."""
    pkg.init(0)
    cache = {}

    def get(name):
        if name not in cache:
            method, rec, lig, kw = case_kwargs(name, orc, table)
            hip = pkg.Scorer.from_pdb(method, rec, lig, **kw)
            assert hip.kernel_info()["pair_kernel_name"] == "dfire_bm_pairs"
            cpu = orc.Scorer(method, rec, lig, **kw)
            base = case_positions(name, orc)
            shifted = table.copy()
            shifted[7::20] += 0.25   # (bin 7 of the 20, every pair of types)
            cpu_shifted = orc.Scorer(method, rec, lig, **dict(kw, potential=shifted))
            pose = base[COPIED[name][0]]
            assert cpu_shifted.energy_row(pose) != cpu.energy_row(pose), name
            known = {}

            def reference(poses):
                for p in poses:
                    if p.tobytes() not in known:
                        e, stats = cpu.energy_ex_row(p)
                        known[p.tobytes()] = (e, int(stats[5]))
                return (np.array([known[p.tobytes()][0] for p in poses]),
                        np.array([known[p.tobytes()][1] for p in poses], dtype=np.int64))
            cache[name] = (hip, reference, base)
        return cache[name]
    return get


def _check(hip, reference, poses, label, monkeypatch, tmp_path, long_drain):
    poses = np.ascontiguousarray(poses)
    got, cnt = _energies_and_counts(hip, poses)
    want, stats = reference(poses)
    err = bm_err(got, want)
    d1 = _debug_record(monkeypatch, tmp_path, hip, poses)
    d2 = _debug_record(monkeypatch, tmp_path, hip, poses)
    pairs, longest = int(d1[:, W_PAIRS].sum()), int(d1[:, W_MAX_TRIPS].max())
    print("%s: bm_err %.2e; drains %d, trips %d, pairs evaluated %d, longest drain %d trips" % (
        label, err, d1[:, W_DRAINS].sum(), d1[:, W_TRIPS].sum(), pairs, longest))
    assert err < REL_TOL, label
    assert np.array_equal(cnt, stats), label
    assert pairs > 0 and pairs == int(d2[:, W_PAIRS].sum()), (label, pairs, int(d2[:, W_PAIRS].sum()))
    assert np.all(d1[:, W_TRIPS] >= d1[:, W_DRAINS]) and d1[:, W_TRIPS].sum() * 256 >= pairs, label   # (a trip: 256 pairs at most)
    if long_drain:
        assert longest >= 3, (label, longest)


@pytest.mark.parametrize("part_cap", [None, "64"], ids=["default", "part_cap_64"])
@pytest.mark.parametrize("name", ["1ppe", "1k4c"])
def test_copies_rigid(drain_case, name, part_cap, monkeypatch, tmp_path):
    """Cases 1, 2 and 4: copies of one pose, with and without short jobs, every launch a counting launch as well."""
    hip, reference, base = drain_case(name)
    if part_cap:
        monkeypatch.setenv("LIGHTDOCK_BM_PART_CAP", part_cap)
    pose, other = base[COPIED[name][0]], base[COPIED[name][1]]
    for n in (1, 63, 64, 65, 300, 1024):
        _check(hip, reference, np.repeat(pose[None], n, axis=0), "%s %s %d copies" % (name, part_cap, n), monkeypatch, tmp_path, n >= 300)
    among = np.repeat(pose[None], 256, axis=0)
    among[101] = other
    _check(hip, reference, among, "%s %s one among 255" % (name, part_cap), monkeypatch, tmp_path, False)


@pytest.mark.parametrize("part_cap", [None, "64"], ids=["default", "part_cap_64"])
def test_anm_with_wild_poses(drain_case, part_cap, monkeypatch, tmp_path):
    """Cases 3 and 4: the ANM form (2uuy): 96 example poses and poses whose amplitudes are forty times their size (wild:
    every pair of theirs goes through bm_recheck to the exact path), copies of the pose with the most pairs, copies of a wild one."""
    hip, reference, base = drain_case("2uuy")
    if part_cap:
        monkeypatch.setenv("LIGHTDOCK_BM_PART_CAP", part_cap)
    wild = base[:40].copy()
    wild[::5, 7:] *= 40.0
    pose = base[COPIED["2uuy"][0]]
    for label, poses, long_drain in (("96 + wild 40", np.concatenate([base[:96], wild]), True), ("one wild pose", wild[:1], False),
                                     ("300 copies", np.repeat(pose[None], 300, axis=0), False),
                                     ("70 wild copies", np.repeat(wild[5:6], 70, axis=0), False)):
        _check(hip, reference, poses, "2uuy %s %s" % (part_cap, label), monkeypatch, tmp_path, long_drain)
