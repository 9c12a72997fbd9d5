"""An `ld_complex*` handle's results do not depend on what it ran or refused before, on the MI355X: the histories of
tests/handle_history.py played to one handle (or two), every call held to the expectation the restatements gave it --
every integer output exactly, the coordinates, the SAXS intensities and the two RMSDs within the bound their own feature's
GPU test applies (imported, no number of this file's) -- and every occurrence of a configured call to the bits of its first
occurrence this session.  A refused call is refused with LD_ERR_INVALID and leaves the handle able to answer.  Every test
but the growth one begins with the soak: every decoy once, so that every shared buffer is larger than any probe needs and
holds another call's data.  tests/test_handle_history_cpu.py proves that the expectations can be missed."""
import numpy as np
import pytest

import handle_history as hh
from test_gpu_analysis import COORDINATES_TOLERANCE
from test_gpu_assess import assert_within_bounds
from test_gpu_saxs import OWN_TABLES_RTOL

pytestmark = pytest.mark.gpu

FIRST = {}      # call name -> the bytes of its first answer this session, on whichever handle


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The files, the configured calls and, computed here once for every test of the module, what the restatements expect
    of every decoy and every probe."""
    w = hh.World(tmp_path_factory.mktemp("history"))
    for handle in hh.HANDLES:
        for step in w.soak(handle) + w.probes(handle):
            w.expected(step.call)
    return w


def held(call, got, want):
    """The library's answer to a configured call against its expectation."""
    if call.entry == "assess":
        assert set(got) == {"kept", "fnat", "irmsd", "lrmsd"} and got["kept"].shape == want["kept"].shape
        for i, m in enumerate(want["_measures"]):
            assert_within_bounds(got, i, m, want["_rs"])
        return
    want = {k: v for k, v in want.items() if not k.startswith("_")}
    assert set(got) == set(want), call.name
    for k, w in want.items():
        g = got[k]
        assert g.shape == w.shape, (call.name, k, g.shape, w.shape)
        if call.entry == "coordinates":
            assert np.max(np.abs(g - w)) < COORDINATES_TOLERANCE, call.name
        elif (call.entry, k) == ("saxs", "intensity"):
            assert np.abs(g - w).max() <= OWN_TABLES_RTOL * np.abs(w).max(), call.name
        else:
            assert g.dtype.kind in "biu" and np.array_equal(g, w.astype(g.dtype)) and np.array_equal(g.astype(w.dtype), w), (call.name, k)


def play(pkg, world, scratch, steps):
    pkg.init(0)
    handles = {}
    for step in steps:
        call = step.call
        if call.handle not in handles:
            handles[call.handle] = world.make_complex(pkg, call.handle)
            assert handles[call.handle].pose_len == world.pose_len[call.handle]
        cx = handles[call.handle]
        if step.expect == hh.REFUSED:
            with pytest.raises(pkg.LightdockError) as e:
                world.run(pkg, cx, call, scratch)
            assert e.value.status == -1, call.name
            continue
        got = world.run(pkg, cx, call, scratch)
        held(call, got, world.expected(call))
        bits = {k: (v.dtype.str, v.shape, v.tobytes()) for k, v in got.items()}
        assert FIRST.setdefault(call.name, bits) == bits, call.name


@pytest.mark.parametrize("x", hh.ENTRIES)
@pytest.mark.parametrize("handle", hh.HANDLES)
def test_every_probe_after_a_decoy_of(pkg, world, tmp_path, handle, x):
    """One row of history 2: decoy(X), probe(Y) for every Y."""
    play(pkg, world, tmp_path, world.soak(handle) + world.pair_row(handle, x))


@pytest.mark.parametrize("how", ("far",) + hh.ARGUMENT_REFUSALS)
@pytest.mark.parametrize("handle", hh.HANDLES)
def test_every_probe_after_a_refused_decoy(pkg, world, tmp_path, handle, how):
    """History 3: a pose beyond the coordinate bound (found by the kernels, after they wrote), a stride below the pose
    length, a NaN, a zero quaternion (found on the host)."""
    play(pkg, world, tmp_path, world.soak(handle) + world.refusals(handle, how))


@pytest.mark.parametrize("handle", hh.HANDLES)
def test_a_refused_reference_leaves_none_and_a_good_one_follows(pkg, world, tmp_path, handle):
    play(pkg, world, tmp_path, world.soak(handle) + world.refused_reference_history(handle))


@pytest.mark.parametrize("handle", hh.HANDLES)
def test_flips_inside_an_entry(pkg, world, tmp_path, handle):
    """History 4, twice over: the second round meets what the first left."""
    play(pkg, world, tmp_path, world.soak(handle) + world.flip_history(handle) + world.flip_history(handle))


@pytest.mark.parametrize("handle", hh.HANDLES)
def test_growth_on_a_fresh_handle(pkg, world, tmp_path, handle):
    """History 5: every probe, every decoy, every probe; no soak."""
    play(pkg, world, tmp_path, world.growth(handle))


def test_two_handles_and_shared_maps(pkg, world, tmp_path):
    """History 6: both handles turn by turn; the Density objects are the same for both."""
    play(pkg, world, tmp_path, [s for pair in zip(world.soak("flex"), world.soak("rigid")) for s in pair] + world.two_handles())
