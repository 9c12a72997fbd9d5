"""The DFIRE pair kernels against the oracle ON the knife edges of their decisions (run with -m gpu on an MI355X): the poses of
tests/dfire_edges.py -- per geometry 3 rotations x 22 edges (20 bin steps, the interface distance, the cutoff) x 42 rungs from
one ulp to beyond a LUT cell either side of the edge, every edge found by bisection on the oracle itself
(tests/test_dfire_edges_cpu.py holds, on the oracle alone, that each is realised).  One value of the staircase table in a
pose's sum is 0.0157 in the energy, seven orders above the tolerance: a pair binned from an f32 distance that an error bound
did not cover fails here.

Routes: the default (block-major `dfire_bm_*`, where bm_accepts takes the complex), LIGHTDOCK_DFIRE_KERNEL=packed with
LIGHTDOCK_PACKED_CELLS 1 and 2, and LIGHTDOCK_DFIRE_KERNEL=allpairs as the all-f64 control.  Per geometry and route: complex A
(no restraints, staircase) and complex B (the targets' residues as restraints, the staircase with a zero last bin: elision
active), all poses in one energy_batch and one counting launch.  Measures: test_gpu_parity.py's own (bm_err on the block-major
route, rel_err elsewhere) below its REL_TOL; in-cutoff pair counts equal the oracle's stats[5], pose by pose.

The f32 answer is what gets compared (block-major route, complex A): with LIGHTDOCK_BM_DEBUG, column 22 of the waves' records
counts the pairs evaluated by the exact path.  The rungs further than max(4, 1 + 1.5 eps) LUT cells from every step and from the
cutoff -- the LUT flags cells within 1/2 + eps of a step, the f32 distance is off by eps / 2 at most -- evaluate as many pairs
exactly as the same poses with the target pair moved 40 A out of range; rho0 and rho1 of every step and of the cutoff evaluate
at least one pair a pose.  A route that sent everything to f64 would pass the comparisons above and fail this.
"""
import numpy as np
import pytest

import dfire_edges
from dfire_edges import GEOMETRIES, N_RUNGS, RUNG_KS
from test_gpu_parity import REL_TOL, BM_ATOL, _counts_of, bm_err, rel_err

pytestmark = pytest.mark.gpu

BM, PACKED = "dfire_bm_pairs", "dfire_packed_pairs"
ROUTES = {"default": {}, "packed1": {"LIGHTDOCK_DFIRE_KERNEL": "packed", "LIGHTDOCK_PACKED_CELLS": "1"},
          "packed2": {"LIGHTDOCK_DFIRE_KERNEL": "packed", "LIGHTDOCK_PACKED_CELLS": "2"}, "allpairs": {"LIGHTDOCK_DFIRE_KERNEL": "allpairs"}}
W_PAIRS = 22


@pytest.fixture(scope="module")
def built(pkg, orc, table, tmp_path_factory):
    pkg.init(0)
    directory = str(tmp_path_factory.mktemp("dfire_edges"))
    return lambda name: dfire_edges.geometry(pkg, orc, table, directory, name)


def _scorer(pkg, monkeypatch, g, which, route):
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    try:
        return pkg.Scorer.from_pdb("dfire", g.rec_pdb, g.lig_pdb, **g.kwargs[which])
    finally:
        for k in ROUTES[route]:
            monkeypatch.delenv(k)


def _expected_kernel(g, route):
    if route == "default":
        return BM if g.frames["bm"]["takes"] else PACKED
    return PACKED if route.startswith("packed") else None


def _per_pose(got, want, block_major):
    """The measure of test_gpu_parity.py, pose by pose (its maximum is bm_err / rel_err)."""
    d = np.abs(got - want)
    return np.maximum(d - BM_ATOL, 0.0) / np.maximum(np.abs(want), 1e-9) if block_major else d / np.maximum(np.abs(want), 1e-9)


def _check_route(pkg, monkeypatch, g, route):
    torch = pytest.importorskip("torch")
    for which in "AB":
        hip = _scorer(pkg, monkeypatch, g, which, route)
        kernel = hip.kernel_info()["pair_kernel_name"]
        want_kernel = _expected_kernel(g, route)
        assert kernel == want_kernel if want_kernel else kernel not in (BM, PACKED), (g.name, route, kernel)
        measure = bm_err if kernel == BM else rel_err
        for batch in g.batches:
            poses, want, counts = g.poses[batch], g.energy[batch, which], g.count[batch, which]
            got = hip.energy_batch(poses)
            counted, got_counts = _counts_of(torch, hip, poses.copy())
            for label, e in (("energy_batch", got), ("counting launch", counted)):
                per = _per_pose(e, want, kernel == BM)
                worst = int(np.argmax(per))
                print("%s %s complex %s %s %s: %s %.2e" % (g.name, route, which, batch, label, measure.__name__, measure(e, want)))
                assert measure(e, want) < REL_TOL, "%s, route %s (%s), complex %s, %s: got %.17g, oracle %.17g; %d poses off" % (
                    g.label(worst), route, kernel, which, label, e[worst], want[worst], int((per >= REL_TOL).sum()))
            off = np.flatnonzero(got_counts.astype(np.int64) != counts)
            assert off.size == 0, "%s, route %s (%s), complex %s: %d pairs counted, the oracle counts %d; %d poses off" % (
                g.label(off[0]), route, kernel, which, got_counts[off[0]], counts[off[0]], off.size)


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("name", GEOMETRIES)
def test_edges_against_the_oracle(built, pkg, monkeypatch, name, route):
    _check_route(pkg, monkeypatch, built(name), route)


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_edges_with_normal_modes(built, pkg, monkeypatch, route):
    """G3anm: 3 + 3 modes that move the targets 0.9 x 16 A along one coordinate, and a batch just above 16 A (WILD)."""
    g = built("G3anm")
    assert g.frames["bm"]["takes"]
    _check_route(pkg, monkeypatch, g, route)


def test_one_frame_beyond_the_largest_is_declined(built, pkg, monkeypatch):
    """G5 is the last frame bm_accepts takes (eps < 8 cells); G6, 1/8 A wider, runs the pose-major kernel -- and is held to the
    oracle on it."""
    g5, g6 = built("G5"), built("G6")
    assert _scorer(pkg, monkeypatch, g5, "A", "default").kernel_info()["pair_kernel_name"] == BM
    assert _scorer(pkg, monkeypatch, g6, "A", "default").kernel_info()["pair_kernel_name"] == PACKED
    _check_route(pkg, monkeypatch, g6, "default")


def test_a_subtile_wider_than_the_bound_covers_is_declined(built, pkg, monkeypatch):
    """W5: a receptor of two groups of four atoms 400 A either side of its one subtile's centre.  The distance arithmetic around
    that centre runs into 2^25 record units squared; bm_accepts measures the subtile, the bound reaches 8 cells, and the complex runs
    the pose-major kernel.  (Taken by the block-major route -- as it was while the bound assumed compact subtiles -- 560 of these
    energies and 100 of the pair counts were wrong on the MI355X.)"""
    g = built("W5")
    assert not g.frames["bm"]["takes"]
    _check_route(pkg, monkeypatch, g, "default")
    _check_route(pkg, monkeypatch, g, "allpairs")


def _exact_pairs(monkeypatch, tmp_path, hip, poses):
    """Pairs the exact path evaluated in one more call with LIGHTDOCK_BM_DEBUG set (tests/test_gpu_bm_exact_drain.py)."""
    path = tmp_path / "bm_debug.txt"
    monkeypatch.setenv("LIGHTDOCK_BM_DEBUG", str(path))
    try:
        hip.energy_batch(np.ascontiguousarray(poses))
    finally:
        monkeypatch.delenv("LIGHTDOCK_BM_DEBUG")
    text = path.read_text() if path.exists() else ""
    path.unlink(missing_ok=True)
    if not text.strip():
        return 0   # (no wave drew a job)
    return int(np.atleast_2d(np.loadtxt(text.splitlines()))[:, W_PAIRS].sum())


@pytest.mark.parametrize("name", GEOMETRIES)
def test_the_f32_answer_is_what_gets_compared(built, pkg, monkeypatch, tmp_path, name):
    g = built(name)
    if not g.frames["bm"]["takes"]:
        pytest.fail("%s is not a block-major complex" % name)
    hip = _scorer(pkg, monkeypatch, g, "A", "default")
    assert hip.kernel_info()["pair_kernel_name"] == BM
    poses = g.poses["rigid"]
    eps = g.frames["bm"]["eps"]
    far = g.cells_from_a_step(pkg) > max(4.0, 1.0 + 1.5 * eps)
    k = len(RUNG_KS)
    rungs = np.arange(len(poses)) % N_RUNGS
    edge = (np.arange(len(poses)) // N_RUNGS) % 22
    on_edge = ((rungs == k) | (rungs == k + 1)) & (edge != 20)            # rho0, rho1 of the steps and the cutoff
    # (a rung 2^-6 A from an edge at r is 2 r cells from it: far at r >= 2 A for eps < 2, at r >= 4 A in G5's frame)
    assert far.sum() >= 90 and on_edge.sum() == 3 * 21 * 2 and not (far & on_edge).any()
    away = poses[far].copy()
    away[:, :3] += 40.0 * g.u
    baseline = _exact_pairs(monkeypatch, tmp_path, hip, away)
    got_far = _exact_pairs(monkeypatch, tmp_path, hip, poses[far])
    got_edge = _exact_pairs(monkeypatch, tmp_path, hip, poses[on_edge])
    print("%s: eps %.3f cells; %d rungs far from every step: %d pairs exact (target out of range: %d); %d rungs on an edge: %d pairs exact"
          % (name, eps, far.sum(), got_far, baseline, on_edge.sum(), got_edge))
    assert np.all(g.count["rigid", "A"][far] <= 1) and g.cpu["A"].energy_ex_row(away[0])[1][5] == 0
    assert got_far == baseline, "%s: %d target pairs far from every step went through the exact path" % (name, got_far - baseline)
    assert got_edge >= on_edge.sum(), (name, got_edge)
