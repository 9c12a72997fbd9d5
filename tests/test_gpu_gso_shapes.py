"""The GSO movement kernels (gso_step.hip) against the oracle at the shapes of tests/gso_shapes.py: ANM rows of 2 + 3, 10 + 0,
0 + 10 and 64 + 64 modes in BOTH kernels (the thread-per-glowworm one never moved an ANM row in a test before), shares of a swarm
larger than a workgroup -- second and third trips of the main loops, partly filled, the phased kernel's second walk with its wave
votes shared by groups without a glowworm --, dynamic LDS up to the limit and the fall-back beyond it, and the refusal of a swarm
that no kernel can hold.  tests/test_gso_shapes_cpu.py shows on the oracle alone that these inputs reach those paths and that
every decision of the reference (`l_i < l_j`, `d < vr_i`) is further from its knife edge than the tolerances here, so integers
are compared for equality.  The roulette's margin |sum - rnd| is NOT checked there: the oracle does not expose the draw; a
target that differed by a rounding of the running sum would show here as an unequal `target`.

Tolerances are those of test_gpu_parity.py: energies and luciferins REL_TOL = 1e-9 (`bm_err` where the block-major DFIRE path
scores, `rel_err` elsewhere), poses 1e-12 absolute (device and host libm differ in `acos` and `sin`), everything integer and the
vision range equal; the kernels among themselves bit for bit.
"""
import numpy as np
import pytest

import gso_shapes
from gso_shapes import CASES, STATE_KEYS, launch, sampled_swarms
from test_gpu_parity import REL_TOL, _k2_env, bm_err, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shapes(pkg, orc, table, tmp_path_factory):
    pkg.init(0)
    return gso_shapes.shapes(pkg, orc, table, str(tmp_path_factory.mktemp("gso_shapes")))


def _against_oracle(hip, got, want, where):
    err = bm_err if hip.kernel_info()["pair_kernel_name"] == "dfire_bm_pairs" else rel_err
    figures = (err(got["scoring"], want["scoring"]), err(got["luciferin"], want["luciferin"]), np.max(np.abs(got["poses"] - want["poses"])))
    print("%s: scoring %.2e luciferin %.2e poses %.2e" % ((where,) + figures))
    for k in ("n_neighbors", "target", "moved", "vision_range"):
        assert np.array_equal(got[k], want[k]), (where, k)
    assert figures[0] < REL_TOL and figures[1] < REL_TOL, where
    assert got["poses"].shape == want["poses"].shape and figures[2] < 1e-12, where


def _bit_identical(a, b, where):
    for k in STATE_KEYS:
        assert np.array_equal(a[k], b[k]), (where, k)


def _single_swarm_case(shapes, monkeypatch, case, every_step):
    c = CASES[case]
    hip = shapes.hip(c["modes"])
    positions, seeds = shapes.swarms(case)
    want = shapes.replay(case)[0]
    assert positions.shape == (1, c["N"], 7 + (sum(c["modes"]) if c["modes"] else 0))
    finals = []
    for k2 in c["k2"]:
        _k2_env(monkeypatch, k2)
        gso = shapes.pkg.GSO(hip, positions, seeds=seeds)
        for step in range(1, c["steps"] + 1):
            gso.step()
            if every_step or step == c["steps"]:
                _against_oracle(hip, gso.read(0), want[step], "%s K2=%s step %d" % (case, k2, step))
        assert gso.num_evals == want[-1]["num_evals"], (case, k2)
        assert gso.steps_done == c["steps"]
        finals.append(gso.read(0))
        gso.close()
    for k2, other in zip(c["k2"][1:], finals[1:]):
        _bit_identical(finals[0], other, "%s K2=%s against unset" % (case, k2))


@pytest.mark.parametrize("case", ["A1", "A2", "A3", "A4", "A5"])
def test_anm_rows_in_both_kernels(shapes, monkeypatch, case):
    """One swarm of a flexing complex, step by step in the three K2 settings (unset runs the phased kernel here, `single` the
    thread-per-glowworm one): few modes, one rigid side, the 64 + 64 modes that fill anm_step's array; 130 glowworms (verdicts
    kept, three words) and 300 (the roulette's second walk)."""
    assert launch(1, CASES[case]["N"], None)["kernel"] == "phased" and launch(1, CASES[case]["N"], "single")["kernel"] == "single"
    _single_swarm_case(shapes, monkeypatch, case, every_step=True)


@pytest.mark.parametrize("case", ["B1", "B2", "B3"])
def test_shares_larger_than_a_workgroup(shapes, monkeypatch, case):
    """Many swarms whose shares take more than one trip of a kernel's main loop.  B1 (512 x 1030) and B2 (256 x 2100, 67 200 B of
    LDS): the thread-per-glowworm kernel, as the launch's own choice beyond 65 536 glowworms and forced -- second trips of 6 and
    26 threads.  B3 (128 x 1030): the phased kernel, trips of 128 / 128 / 2 glowworms on its second walk, and the other kernel
    to compare with.  Swarms 0, S/2 and S-1 against the oracle after the run; swarms 1 and S-1, the same positions and seed, bit for
    bit; the settings among themselves bit for bit on the sampled swarms."""
    c = CASES[case]
    hip = shapes.hip(None)
    positions, seeds = shapes.swarms(case)
    want = shapes.replay(case)
    last = c["S"] - 1
    runs = []
    for k2 in c["k2"]:
        assert launch(c["S"], c["N"], k2)["kernel"] == c["expect"][k2]["kernel"]
        _k2_env(monkeypatch, k2)
        gso = shapes.pkg.GSO(hip, positions, seeds=seeds)
        gso.run(c["steps"])
        got = {s: gso.read(s) for s in sampled_swarms(case)}
        _bit_identical(gso.read(1), got[last], "%s K2=%s swarms 1 and %d" % (case, k2, last))
        gso.close()
        for s in sampled_swarms(case):
            _against_oracle(hip, got[s], want[s][-1], "%s K2=%s swarm %d" % (case, k2, s))
        runs.append(got)
    for s in sampled_swarms(case):
        _bit_identical(runs[0][s], runs[1][s], "%s swarm %d: %s against %s" % (case, s, c["k2"][0], c["k2"][1]))


@pytest.mark.parametrize("case", ["C1", "C2", "C3"])
def test_lds_limits(shapes, monkeypatch, case):
    """One swarm at the limits of a CU's LDS: 3413 glowworms, the most the phased kernel holds (163 824 of 163 840 B); 3414, for
    which the thread-per-glowworm kernel runs whatever is asked for; 4096, the largest swarm admitted (131 072 B).  After the
    last step against the oracle, the three settings bit for bit."""
    _single_swarm_case(shapes, monkeypatch, case, every_step=False)


def test_a_swarm_of_more_than_4096_glowworms_is_refused(shapes):
    hip = shapes.hip(None)
    batch = shapes.pkg.synth.swarm(24, seed=7)
    before = hip.energy_batch(batch)
    with pytest.raises(shapes.pkg.LightdockError, match="4096"):
        shapes.pkg.GSO(hip, shapes.pkg.synth.swarm(4097, seed=1))
    assert np.array_equal(hip.energy_batch(batch), before)
