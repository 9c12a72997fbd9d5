"""What makes the histories of tests/handle_history.py able to fail, proved on the restatements alone (no GPU, no library):
history 2 holds every ordered pair of entries once; a probe that returned what its decoy left behind, or read one pose row
or one score of its decoy's, would miss its expectation; no probe is trivial; every decoy is large enough to leave every
shared buffer larger than any probe needs.  These are conditions on the chosen inputs, not measurements."""
import collections

import numpy as np
import pytest

import handle_history as hh
import sasa_reference as sr
import xlink_reference as xr


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return hh.World(tmp_path_factory.mktemp("history"))


def arrays(expected):
    return {k: v for k, v in expected.items() if not k.startswith("_")}


def differs(a, b):
    """Two expectations of one call shape differ in at least one array."""
    a, b = arrays(a), arrays(b)
    assert a.keys() == b.keys()
    return any(x.shape != b[k].shape or not np.array_equal(x, b[k]) for k, x in a.items())


def test_history_2_holds_every_ordered_pair_exactly_once(world):
    for handle in hh.HANDLES:
        steps = world.pairs(handle)
        seen = collections.Counter()
        for before, after in zip(steps[::2], steps[1::2]):
            assert before.call.kind == "decoy" and after.call.kind == "probe" and before.call.handle == after.call.handle == handle
            assert before.expect == after.expect == hh.OK
            seen[(before.call.entry, after.call.entry)] += 1
        assert len(hh.ENTRIES) == 16 and len(seen) == len(hh.ENTRIES) ** 2 and set(seen.values()) == {1}
        assert set(seen) == {(x, y) for x in hh.ENTRIES for y in hh.ENTRIES}
        for x in hh.ENTRIES:        # a row is a test: one X, every Y
            row = world.pair_row(handle, x)
            assert [s.call.entry for s in row[::2]] == [x] * 16 and [s.call.entry for s in row[1::2]] == list(hh.ENTRIES)


@pytest.mark.parametrize("handle", hh.HANDLES)
def test_a_probe_that_returned_its_decoys_output_would_fail(world, handle):
    for entry in hh.ENTRIES:
        probe, decoy = (world.expected(world.call(entry, kind, handle)) for kind in ("probe", "decoy"))
        assert arrays(probe) and set(arrays(probe)) <= set(arrays(decoy)), entry
        for name, want in arrays(probe).items():
            stale, mine = hh.leading(decoy[name], want)
            assert mine.size and not np.array_equal(stale, mine), (entry, name)


@pytest.mark.parametrize("handle", hh.HANDLES)
def test_a_probe_that_read_a_pose_row_or_a_score_of_its_decoys_would_fail(world, handle):
    L = world.pose_len[handle]
    for entry in hh.ENTRIES:
        probe, decoy = world.call(entry, "probe", handle), world.call(entry, "decoy", handle)
        if probe.poses is None:
            continue                # set_reference reads no pose
        want = world.expected(probe)
        mine, theirs = probe.poses.reshape(-1, probe.poses.shape[-1]), decoy.poses.reshape(-1, decoy.poses.shape[-1])
        for i in range(len(mine)):
            rows = mine.copy()
            rows[i, :L] = theirs[i, :L]
            assert differs(world._compute(probe._replace(poses=rows.reshape(probe.poses.shape))), want), (entry, "pose", i)
        if probe.scores is not None:
            for i in range(probe.scores.size):
                scores = probe.scores.copy()
                scores.reshape(-1)[i] = decoy.scores.reshape(-1)[i]
                assert differs(world._compute(probe._replace(scores=scores)), want), (entry, "score", i)


@pytest.mark.parametrize("handle", hh.HANDLES)
def test_no_probe_is_trivial(world, handle):
    def probe(entry):
        call = world.call(entry, "probe", handle)
        return call, world.expected(call)

    rs = world.rs[handle]
    call, _ = probe("sasa")
    _, free, bound = sr.SasaRestated.batch(rs.xlink, call.poses, call.params["probe"])
    assert (bound < free).any() and ((bound == free) & (free > 0)).any() and (bound > 0).any()       # buried by the other molecule, and not
    _, want = probe("contacts")
    assert want["rec"].any() and not want["rec"].all() and want["lig"].any()
    call, want = probe("pair_contacts")
    assert 0 < len(want["keys"]) < len(call.poses) * hh.N_REC_RES * hh.N_LIG_RES
    call, want = probe("crosslinks")
    assert (want["path"] == xr.NO_PATH).any() and (want["path"] != xr.NO_PATH).any()
    assert hh.xlink_bits_in_lds(call.params["max_length"], call.params["cell"])
    decoy = world.call("crosslinks", "decoy", handle)
    assert not hh.xlink_bits_in_lds(decoy.params["max_length"], decoy.params["cell"])
    assert len(set(decoy.params["links"][:, 0])) != len(set(call.params["links"][:, 0]))              # another source grouping
    call, _ = probe("ccs")
    sums = [rs.ccs.batch(call.poses, what, call.params["probe"], call.params["cell"])[1] for what in (0, 1, 2)]
    assert all((sums[a] != sums[b]).all() for a, b in ((0, 1), (0, 2), (1, 2)))
    for entry in ("cluster", "cluster_ranked", "cluster_fcc"):
        call, want = probe(entry)
        n = call.scores.shape[-1]
        assert (1 < want["n_clusters"]).all() and (want["n_clusters"] < n).all(), entry
    _, want = probe("cluster_fcc")
    assert np.bincount(want["cluster_of"][want["cluster_of"] >= 0]).max() >= 2 and (want["set_sizes"] > 0).all()
    _, want = probe("assess")
    native = len(want["_rs"].native)
    assert native > 0 and any(want["kept"][i] > 0 and want["kept"][j] < native for i in range(len(want["kept"])) for j in range(len(want["kept"])) if i != j)
    for entry in ("density_fit", "simulate_density"):
        call, want = probe(entry)
        fit = world.expected(world.call("density_fit", "probe", handle)) if entry == "density_fit" else None
        if fit is not None:
            assert (fit["outside"] > 0).any() and (fit["inside_sum"] > 0).all() and (fit["inside_sum"] < fit["s"]).all()
        else:
            assert want["grid"].any()
    _, want = probe("distance_histogram")
    assert want["counts"].any()
    # reference B lacks two receptor residues and one ligand residue
    a, b = (world.expected(world.call("set_reference", kind, handle))["counts"] for kind in ("probe", "decoy"))
    assert (int(a[0]) - int(b[0]), int(a[1]) - int(b[1])) == (2 * len(hh.RESIDUE), len(hh.RESIDUE)) and a[2] > 0 and b[2] > 0


def test_every_decoy_asks_for_eight_times_its_probes_poses_and_every_optional_output(world):
    for handle in hh.HANDLES:
        for entry in hh.ENTRIES:
            probe, decoy = world.call(entry, "probe", handle), world.call(entry, "decoy", handle)
            if entry in hh.SINGLE:
                continue
            n_probe, n_decoy = (int(np.prod(c.poses.shape[:-1])) for c in (probe, decoy))
            assert 1 <= n_probe <= 4 and n_decoy >= 8 * n_probe, entry
            assert decoy.poses.shape[-1] > world.pose_len[handle] == probe.poses.shape[-1]             # a stride wider than the pose
            assert any(not np.array_equal(np.asarray(decoy.params[k]), np.asarray(v)) for k, v in probe.params.items()) or not probe.params, entry
            assert set(arrays(world.expected(probe))) <= set(arrays(world.expected(decoy)))
        on = {"sasa": "atoms", "ccs": "views", "crosslinks": "paths", "saxs": "counts"}
        assert all(world.call(e, "decoy", handle).params[flag] is True for e, flag in on.items())
        assert world.call("density_fit", "decoy", handle).params["map"] != world.call("density_fit", "probe", handle).params["map"]
    assert world.maps["one"][0].shape != world.maps["two"][0].shape


def test_refusal_histories_put_every_probe_behind_every_refused_call(world):
    for handle in hh.HANDLES:
        for how in ("far",) + hh.ARGUMENT_REFUSALS:
            steps = world.refusals(handle, how)
            heads = [i for i, s in enumerate(steps) if s.expect == hh.REFUSED]
            assert heads == list(range(0, len(steps), 17)) and len(steps) % 17 == 0
            refused = [steps[i].call.entry for i in heads]
            want = [e for e in hh.ENTRIES if (e in hh.FAR if how == "far" else e != "set_reference" and (how != "stride" or e != "write_pdb"))]
            assert refused == want, how
            for i in heads:
                assert [s.call.name for s in steps[i + 1:i + 17]] == [s.call.name for s in world.probes(handle)]
                bad, good = steps[i].call, world.call(steps[i].call.entry, "decoy", handle)
                if how == "stride":
                    assert bad.poses.shape[-1] == world.pose_len[handle] - 1
                else:           # the last pose alone is unacceptable
                    flat_bad, flat_good = bad.poses.reshape(-1, bad.poses.shape[-1]), good.poses.reshape(-1, good.poses.shape[-1])
                    assert np.array_equal(flat_bad[:-1], flat_good[:-1]) and not np.array_equal(flat_bad[-1], flat_good[-1], equal_nan=True)
                    if how == "far":
                        posed = world.rs[handle].em.pose(flat_bad[-1])[world.n_rec:]
                        assert np.abs(posed).max() > (2147483.647 if steps[i].call.entry in ("cluster", "cluster_ranked") else 1.0e6)
        history = world.refused_reference_history(handle)
        assert [s.expect for s in history] == [hh.OK, hh.REFUSED, hh.REFUSED, hh.OK, hh.OK]
        assert history[-1].call is world.call("assess", "probe", handle)


def test_flips_growth_and_the_two_handles(world):
    for handle in hh.HANDLES:
        flips = world.flip_history(handle)
        by_entry = collections.defaultdict(list)
        for s in flips:
            by_entry[s.call.entry].append(s.call)
        assert [c.params["atoms"] for c in by_entry["sasa"]] == [True, False, True] and len({len(c.poses) for c in by_entry["sasa"]}) == 3
        assert [(c.params["what"], c.params["cell"]) for c in by_entry["ccs"]] == [(2, 0.5), (0, 0.5), (1, 2.0), (2, 2.0), (2, 0.5)]
        xl = by_entry["crosslinks"]
        assert [c.params["paths"] for c in xl][:2] == [False, True] and len({c.params["links"].tobytes() for c in xl}) == 4
        assert {hh.xlink_bits_in_lds(c.params["max_length"], c.params["cell"]) for c in xl} == {True, False}
        assert {c.params["bins"] for c in by_entry["saxs"]} == {1024, 64} and {c.params["chunk"] for c in by_entry["saxs"]} == {0, 1}
        assert {c.params["bins"] for c in by_entry["distance_histogram"]} == {1024, 64}
        assert [s.call.params["map"] for s in flips if s.call.entry in ("density_fit", "simulate_density")] == ["one", "two", "two", "one", "one"]
        assert [c.params["reference"] for c in by_entry["set_reference"]] == list("ABA") == [c.params["reference"] for c in by_entry["assess"]]
        for s in flips:             # every flip has an expectation of its own
            assert arrays(world.expected(s.call))
        growth = world.growth(handle)
        assert [s.call.kind for s in growth] == ["probe"] * 16 + ["decoy"] * 16 + ["probe"] * 16
    both = world.two_handles()
    assert [s.call.handle for s in both] == list(hh.HANDLES) * 32 and both[0].call.entry == both[1].call.entry == hh.ENTRIES[0]
