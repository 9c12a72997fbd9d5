"""An `ld_scorer*` handle's results do not depend on what it, or an `ld_gso*` that shares it, ran or refused before, on the
MI355X: the histories of tests/scorer_history.py played to freshly built handles.  Every OK call is held to the expectation the
oracle and the restatements gave it (World.held: energies under the handle's own measure of test_gpu_parity.py below REL_TOL,
pair counts, decompositions, refinement histories and poses and every GSO decision exactly) and to the bits of the FRESH
answer: the same configured call made once, in a module fixture, on a newly built handle that has run nothing else.  The second
comparison is what pins DESIGN's "the same bits in every batch" across calls: no tolerance could hide a stale sum, flag or
energy in it.  NaN matches NaN.  A refused call returns LD_ERR_INVALID (LightdockError, status -1), leaves its outputs at
their sentinel and the handle able to answer.  Every test but the growth one begins with the soak: every decoy once, so that
every buffer is larger than any probe needs and holds another call's data.  tests/test_scorer_history_cpu.py proves that the
expectations can be missed."""
import time

import numpy as np
import pytest

import scorer_history as sh
from test_gpu_bm_launch_sequence import _with_env
from test_gpu_gso_shapes import _against_oracle
from test_gpu_refine import same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(pkg, orc, table, tmp_path_factory):
    """The files, the oracles, the configured calls and, computed here once for every test of the module, what every call
    must return."""
    pkg.init(0)
    start = time.perf_counter()
    w = sh.World(orc, table, tmp_path_factory.mktemp("scorer_history"))
    for call in w.calls.values():
        w.expected(call)
    print("scorer_history expectations: %.1f s" % (time.perf_counter() - start))
    return w


def bits_equal(a, b):
    """Two answers to one configured call, to the bit; a NaN matches a NaN (test_gpu_refine.same_bits)."""
    keys = {k for k in a if k != "_got"}
    if keys != {k for k in b if k != "_got"}:
        return False
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype == np.float64:
            if not same_bits(x, y):
                return False
        elif x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            return False
    return True


def snapshot(got):
    return {k: np.array(v) for k, v in got.items() if k != "_got"}


@pytest.fixture(scope="module")
def fresh(pkg, world):
    """(handle, call name) -> the call's answer on a newly built handle that has run nothing else; every configured call of
    every handle, made here once."""
    torch = pytest.importorskip("torch")
    start = time.perf_counter()
    out = {}
    for handle, (complex_, _, _) in sh.HANDLES.items():
        for call in world.calls.values():
            if call.complex == complex_:
                hip = world.make_scorer(pkg, handle, _with_env)
                out[(handle, call.name)] = snapshot(world.run(pkg, torch, hip, call))
                hip.close()
    print("scorer_history fresh answers: %d calls, %.1f s" % (len(out), time.perf_counter() - start))
    return out


SLOWEST = [0.0, None]


@pytest.fixture(scope="module", autouse=True)
def slowest_call():
    yield
    print("scorer_history slowest call: %s, %.3f s" % (SLOWEST[1], SLOWEST[0]))


def answer(pkg, world, fresh, handle, hip, call):
    """One OK call: held to its expectation and to the bits of the fresh answer."""
    torch = pytest.importorskip("torch")
    start = time.perf_counter()
    got = world.run(pkg, torch, hip, call)
    took = time.perf_counter() - start
    if took > SLOWEST[0]:
        SLOWEST[:] = [took, "%s on %s" % (call.name, handle)]
    world.held(handle, hip, call, got)
    assert bits_equal(snapshot(got), fresh[(handle, call.name)]), (handle, call.name, "differs from the fresh handle's bits")


def play(pkg, world, fresh, steps, handles=None):
    """steps: (handle, Step) in the order played; every handle is built fresh when its first step comes (or taken from
    `handles`, which a test passes to go on with the same ones)."""
    torch = pytest.importorskip("torch")
    pkg.init(0)
    handles = {} if handles is None else handles
    for item in steps:
        handle, step = item
        if handle not in handles:
            handles[handle] = world.make_scorer(pkg, handle, _with_env)
        hip = handles[handle]
        if step.expect == sh.OK:
            answer(pkg, world, fresh, handle, hip, step.call)
            continue
        status, untouched = world.refuse(pkg, torch, hip, step.call, step.expect)
        with pytest.raises(pkg.LightdockError) as e:
            pkg._check(status)
        assert e.value.status == -1 and untouched, (handle, step.call.name, step.expect)
    return handles


def on(handle, steps):
    return [(handle, s) for s in steps]


def test_every_handle_reports_its_pair_kernel_and_bm16_runs_70_poses_in_five_passes(pkg, world):
    pkg.init(0)
    for handle, (_, _, kernel) in sh.HANDLES.items():
        hip = world.make_scorer(pkg, handle, _with_env)
        assert hip.kernel_info()["pair_kernel_name"] == kernel
        if handle == "bm16":      # from the pass size the library derived: 16, 16, 16, 16, 6 on two sets; up to 16 one fused pass
            n = len(world.of(handle, "energy_batch", "decoy").poses)
            assert n == 70 and hip.bm_passes(n) == (16, 2) and -(-n // hip.bm_passes(n)[0]) == 5
            assert hip.bm_passes(16) == (16, 1) and hip.bm_passes(17) == (16, 2) and hip.bm_passes(9) == (9, 1)
        elif kernel == "dfire_bm_pairs":
            assert hip.bm_passes(70) == (70, 1) and hip.bm_passes(5) == (5, 1)
        else:
            assert hip.bm_passes(70) == (0, 0)


@pytest.mark.parametrize("x", sh.ENTRIES)
@pytest.mark.parametrize("handle", sh.HANDLES)
def test_every_probe_after_a_decoy_of(pkg, world, fresh, handle, x):
    """One row of history 2: decoy(X), probe(Y) for every Y."""
    play(pkg, world, fresh, on(handle, world.soak(handle) + world.pair_row(handle, x)))


@pytest.mark.parametrize("x", [e for e in sh.ENTRIES if sh.REFUSALS[e]])
@pytest.mark.parametrize("handle", sh.HANDLES)
def test_every_probe_after_the_refused_forms_of(pkg, world, fresh, handle, x):
    """History 3: before every probe a decoy(X) with a stride below the pose length and one without its pose buffer."""
    play(pkg, world, fresh, on(handle, world.soak(handle) + world.refusals(handle, x)))


@pytest.mark.parametrize("handle", sh.HANDLES)
def test_flips_inside_an_entry(pkg, world, fresh, handle):
    """History 4."""
    play(pkg, world, fresh, on(handle, world.soak(handle) + world.flip_history(handle)))


@pytest.mark.parametrize("handle", sh.HANDLES)
def test_growth_on_a_fresh_handle(pkg, world, fresh, handle):
    """History 5: every probe, every decoy, every probe; no soak."""
    play(pkg, world, fresh, on(handle, world.growth(handle)))


def step_and_hold(world, hip, gso, call, upto):
    """One more step of a GSO that stays alive: its state is the oracle's after that many steps."""
    gso.step()
    for s, state in enumerate(world.expected(call)["_steps"][upto - 1]):
        _against_oracle(hip, gso.read(s), state, "%s after %d steps" % (call.name, upto))
    assert gso.steps_done == upto


@pytest.mark.parametrize("handle", sh.HANDLES)
def test_a_gso_that_stays_alive_while_others_use_its_scorer(pkg, world, fresh, handle):
    """History 6: two steps, every decoy (another GSO built, stepped and closed among them; the refinement grows the
    workspace), two more steps.  The state is the oracle's after each of the four steps and ends bit-equal to the probe `gso`
    call of a fresh handle."""
    call = world.of(handle, "gso", "probe")
    handles = play(pkg, world, fresh, on(handle, world.soak(handle)))
    hip = handles[handle]
    gso = world.make_gso(pkg, hip, call)
    for upto in (1, 2):
        step_and_hold(world, hip, gso, call, upto)
    play(pkg, world, fresh, on(handle, world.between(handle)), handles)
    for upto in (3, 4):
        step_and_hold(world, hip, gso, call, upto)
    assert bits_equal(world.gso_outputs(gso), fresh[(handle, call.name)])
    gso.close()


@pytest.mark.parametrize("handle", sh.HANDLES)
def test_two_gsos_on_one_scorer_stepped_turn_by_turn(pkg, world, fresh, handle):
    """History 6, the second half: two probe GSOs of different seeds share one scorer's workspace."""
    calls = [world.of(handle, "gso", kind) for kind in ("probe", "probe2")]
    handles = play(pkg, world, fresh, on(handle, world.soak(handle)))
    hip = handles[handle]
    gsos = [world.make_gso(pkg, hip, call) for call in calls]
    for upto in (1, 2, 3, 4):
        for gso, call in zip(gsos, calls):
            step_and_hold(world, hip, gso, call, upto)
    for gso, call in zip(gsos, calls):
        assert bits_equal(world.gso_outputs(gso), fresh[(handle, call.name)])
        gso.close()


@pytest.mark.parametrize("handle", sh.GRAPH_HANDLES)
def test_graph_replay_between_other_callers(pkg, world, fresh, handle, monkeypatch):
    """History 7: run(8) under LIGHTDOCK_GSO_GRAPH=1, decoys that do not grow the workspace, run(8).  The state after 16 steps
    is the oracle's and bit-equal to 16 eager steps on a fresh handle (the fixture's, made without the variable).  On `dna`
    (1azp has receptor modes) Gso::run keeps plain launches whatever the variable says: there the test holds just that."""
    call = world.of(handle, "gso", "graph")
    handles = play(pkg, world, fresh, on(handle, world.soak(handle)))
    hip = handles[handle]
    monkeypatch.setenv("LIGHTDOCK_GSO_GRAPH", "1")
    gso = world.make_gso(pkg, hip, call)
    gso.run(8)
    assert gso.steps_done == 8
    play(pkg, world, fresh, on(handle, world.quiet_decoys(handle)), handles)
    gso.run(8)
    got = world.gso_outputs(gso)
    gso.close()
    world.held(handle, hip, call, got)
    assert bits_equal(got, fresh[(handle, call.name)])


def test_two_handles_turn_by_turn(pkg, world, fresh):
    """History 8: `bm` and `bm-anm` through one pair row; they share files and nothing else."""
    soak = [item for pair in zip(on("bm", world.soak("bm")), on("bm-anm", world.soak("bm-anm"))) for item in pair]
    play(pkg, world, fresh, soak + world.two_handles())
