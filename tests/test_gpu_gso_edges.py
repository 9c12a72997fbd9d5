"""The GSO movement kernels (gso_step.hip) against the oracle ON the knife edges of their decisions, at the cases of
tests/gso_edges.py: luciferin ties, d == vr and an ulp either side (at step 1 and later), the vision range's clamps at 0 and 5
and the kFarD2 short cut, a glowworm that lands exactly on its target and divides by a zero norm at the next step, the roulette
across the words of the kept verdicts and on the second walk, the 4- and 8-wide scan tails, the slerp's branches at dot ==
0.9995, +-1, +-0, and ANM steps whose squared norm is 0 or inf -- in the three settings of LIGHTDOCK_GSO_K2.
tests/test_gso_edges_cpu.py shows on the oracle alone that every motif sits on its edge at the step it is built for.

Nothing here is a tolerance but one: everything that decides a movement is IEEE f64 with correctly rounded sqrt and /, and the
energies are a staircase of powers of two, so n_neighbors, target, moved, the vision range, scoring, luciferin, translations,
ANM extents and every rotation that did not go through acos / sin are compared BIT FOR BIT, NaNs equal in place, step by step.
Rotations of the slerp branch keep the 1e-12 absolute of test_gpu_gso_shapes._against_oracle (device and host libm differ).
The K2 settings among themselves are bit for bit identical, rotations included.

What a mutated kernel would fail (tests/test_gso_edges_cpu.py::test_a_mutated_restatement_disagrees_with_the_oracle shows the
same mutations against the oracle): `d <= vr` -- E2at in N9, N66, N256, N257, N263 (n_neighbors at step 1); `li <= lj` -- E1
everywhere and every pair of fillers (n_neighbors at step 1); kFarD2 = 24.9 -- E4in in N66, N256, N263 (n_neighbors at step
13); the kept bits' `& 63` as `& 31` -- the fans of N256, N65, N66, N67 whose neighbours are 63 / 64 / 127 / 128 / 191 / 192 /
255 (target, or n_neighbors where two bits fold onto one); `fmax(0.0, v)` dropped -- E5x8 (vision_range after step 1);
the scan tail's `j < j_end` dropped -- the fans with neighbours N-1, N-2, N-3 in N65, N66, N67, N263, if what lies behind the
swarm in LDS happens to look like a neighbour (nothing defines it); `dot >= kLinearThreshold` -- E2in's mover in N2, N9, N256,
N257, N263, one step late: at t = 0.5 the normalised lerp and the slerp are the same point, so at dot == 0.9995 the two branches
differ in the last bits only, inside the 1e-12 owed to libm at that step; the mover's NEXT move takes the linear branch from
that rotation and is compared bit for bit.  (That comparison holds because the device's acos and sin return the host's bits at the
angles used here -- the slerp rotations differ by 0.0 on the MI355X; were a libm ever an ulp off, the rotations downstream of a
slerp step are where it would show first.)
"""
import time

import numpy as np
import pytest

import gso_edges
from gso_edges import CASES, K2_ALL, STEPS, launch, sampled_swarms, same_bits
from test_gpu_parity import _k2_env

pytestmark = pytest.mark.gpu

SINGLE = sorted(c for c in CASES if CASES[c]["S"] == 1)
INT_KEYS = ("n_neighbors", "target", "moved")
F64_KEYS = ("vision_range", "scoring", "luciferin")


@pytest.fixture(scope="module")
def edges(pkg, orc, tmp_path_factory):
    pkg.init(0)
    return gso_edges.edges(pkg, orc, str(tmp_path_factory.mktemp("gso_edges")))


def _against_oracle(got, want, events, where):
    """One swarm after a step: everything bit for bit but the rotations that `events` (the restatement of that step) says went
    through the slerp branch."""
    for k in INT_KEYS:
        assert np.array_equal(got[k], want[k]), (where, k, np.flatnonzero(got[k] != want[k])[:8])
    for k in F64_KEYS:
        assert same_bits(got[k], want[k]), (where, k)
    assert got["poses"].shape == want["poses"].shape
    cols = np.r_[0:3, 7:got["poses"].shape[1]]
    assert same_bits(got["poses"][:, cols], want["poses"][:, cols]), (where, "translations / extents")
    slerp = np.array([events[i].get("branch") == "slerp" for i in range(len(events))])
    assert same_bits(got["poses"][~slerp, 3:7], want["poses"][~slerp, 3:7]), (where, "rotations (linear branch, not moved)")
    a, b = got["poses"][slerp, 3:7], want["poses"][slerp, 3:7]
    assert np.array_equal(np.isnan(a), np.isnan(b)), (where, "rotations (slerp): NaNs")
    worst = float(np.nanmax(np.abs(a - b), initial=0.0))
    assert worst < 1e-12, (where, "rotations (slerp)", worst)
    return worst


def _bit_identical(a, b, where):
    for k in INT_KEYS:
        assert np.array_equal(a[k], b[k]), (where, k)
    for k in F64_KEYS + ("poses",):
        assert same_bits(a[k], b[k]), (where, k)


@pytest.mark.parametrize("case", sorted(CASES))
def test_premise_energies_equal_the_oracle_bit_for_bit(edges, case):
    """One pair, a power of two from the table, the f64 tail of pose_energy_tail.hpp: energy_batch of a case's starting poses IS
    the oracle's, on whichever pair route the scorer runs."""
    c = CASES[case]
    rows, _ = edges.swarm(case)
    hip = edges.hip(c["modes"])
    got, want = hip.energy_batch(rows), edges.cpu(c["modes"]).energy_rows(rows)
    print("EDGES %s: pair route %s, %d distinct energies" % (case, hip.kernel_info()["pair_kernel_name"], len(set(want.tolist()))))
    assert same_bits(got, want), (case, np.flatnonzero(got != want)[:8])


@pytest.mark.parametrize("modes", [None, (1, 1), (3, 2)], ids=["P", "P-anm 1+1", "P-anm 3+2"])
def test_premise_poses_that_are_not_finite_score_as_the_oracle_says(edges, modes):
    """What E6 and E10 leave behind: NaN translations, NaN and infinite extents.  The reference's `dist <= 225` is false for
    them, no pair is counted, the energy is 4.7."""
    k = sum(modes) if modes else 0
    rows = np.zeros((6, 7 + k))
    rows[:, 3] = 1.0
    rows[:, 0] = 3.2
    rows[0, :3] = np.nan
    rows[1, 1] = np.nan
    if modes:
        rows[2, 7:] = np.nan
        rows[3, 7] = np.inf
        rows[4, 7 + modes[0]:] = np.nan
        rows[5, 7 + modes[0]] = np.inf
    got, want = edges.hip(modes).energy_batch(rows), edges.cpu(modes).energy_rows(rows)
    print("EDGES not finite:", got, want)
    assert same_bits(got, want) and want[0] == 4.7 and want[1] == 4.7


@pytest.mark.parametrize("case", SINGLE)
def test_on_the_edges_step_by_step(edges, monkeypatch, case):
    """One swarm in the three K2 settings, every step against the oracle; the settings among themselves bit for bit at every
    step, rotations included."""
    c = CASES[case]
    hip = edges.hip(c["modes"])
    positions, seeds = edges.swarms(case)
    want, restated = edges.replay(case)[0], edges.restate(case, 0)
    history = {}
    for k2 in K2_ALL:
        assert launch(1, c["N"], k2)["kernel"] == c["expect"][k2]["kernel"]
        _k2_env(monkeypatch, k2)
        start = time.perf_counter()
        gso = edges.pkg.GSO(hip, positions, seeds=seeds)
        worst, states = 0.0, []
        for step in range(1, STEPS + 1):
            gso.step()
            states.append(gso.read(0))
            worst = max(worst, _against_oracle(states[-1], want[step], restated[step - 1][5], "%s K2=%s step %d" % (case, k2, step)))
        assert gso.num_evals == want[-1]["num_evals"], (case, k2)
        assert gso.steps_done == STEPS
        gso.close()
        history[k2] = states
        print("EDGES %s K2=%s: %d steps in %.3f s, slerp rotations within %.2e" % (case, k2, STEPS, time.perf_counter() - start, worst))
    for k2 in K2_ALL[1:]:
        for step, (a, b) in enumerate(zip(history[None], history[k2]), 1):
            _bit_identical(a, b, "%s step %d: K2=%s against unset" % (case, step, k2))


def test_many_swarms_on_the_edges(edges, monkeypatch):
    """600 copies of the N = 67 swarm with seeds of their own, one workgroup a swarm (parts = 1): swarms 0, 300 and 599 against
    the oracle at every step, swarms 1 and 599 (the same seed) bit for bit, the settings among themselves."""
    case = "M67"
    c = CASES[case]
    hip = edges.hip(None)
    positions, seeds = edges.swarms(case)
    assert positions.shape == (600, 67, 7) and seeds[1] == seeds[599] and len(set(seeds.tolist())) == 599
    want = edges.replay(case)
    restated = {s: edges.restate(case, s) for s in sampled_swarms(case)}
    finals = {}
    for k2 in K2_ALL:
        assert launch(c["S"], c["N"], k2)["parts"] == 1 and launch(c["S"], c["N"], k2)["kernel"] == c["expect"][k2]["kernel"]
        _k2_env(monkeypatch, k2)
        start = time.perf_counter()
        gso = edges.pkg.GSO(hip, positions, seeds=seeds)
        for step in range(1, STEPS + 1):
            gso.step()
            for s in sampled_swarms(case):
                _against_oracle(gso.read(s), want[s][step], restated[s][step - 1][5], "%s K2=%s swarm %d step %d" % (case, k2, s, step))
            _bit_identical(gso.read(1), gso.read(c["S"] - 1), "%s K2=%s step %d: swarms 1 and %d" % (case, k2, step, c["S"] - 1))
        assert gso.steps_done == STEPS
        finals[k2] = {s: gso.read(s) for s in sampled_swarms(case) + (1, 7)}
        gso.close()
        print("EDGES %s K2=%s: %d steps in %.3f s" % (case, k2, STEPS, time.perf_counter() - start))
    for k2 in K2_ALL[1:]:
        for s in finals[None]:
            _bit_identical(finals[None][s], finals[k2][s], "%s swarm %d: K2=%s against unset" % (case, s, k2))


@pytest.mark.parametrize("case", ["N67", "N257"])
def test_the_nan_glowworm_through_the_captured_graph(edges, monkeypatch, case):
    """The E6 cases once through ld_gso_run with LIGHTDOCK_GSO_GRAPH=1 (two captured steps a replay): the same bits as stepping,
    and the oracle's."""
    assert any(m[0] == "E6" for m in gso_edges.motifs_of(case))
    monkeypatch.setenv("LIGHTDOCK_GSO_GRAPH", "1")
    _k2_env(monkeypatch, None)
    c = CASES[case]
    hip = edges.hip(c["modes"])
    positions, seeds = edges.swarms(case)
    a, b = edges.pkg.GSO(hip, positions, seeds=seeds), edges.pkg.GSO(hip, positions, seeds=seeds)
    a.run(STEPS)
    for _ in range(STEPS):
        b.step()
    sa, sb = a.read(0), b.read(0)
    assert a.steps_done == STEPS and a.num_evals == b.num_evals == edges.replay(case)[0][-1]["num_evals"]
    a.close()
    b.close()
    _bit_identical(sa, sb, "%s: the captured graph against stepping" % case)
    _against_oracle(sa, edges.replay(case)[0][STEPS], edges.restate(case, 0)[STEPS - 1][5], "%s: the captured graph" % case)
    nan = np.isnan(sa["poses"][:, 0])
    assert nan.sum() >= 1 and (sa["scoring"][nan] == 4.7).all()
