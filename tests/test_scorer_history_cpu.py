"""What makes the histories of tests/scorer_history.py able to fail, proved on the oracle and the restatements alone (no GPU, no
library call): a probe that returned what any decoy left behind would miss its expectation in every element that carries
information; the far probe pose has no pair within the cutoff and scores the bare constant; every tail term a complex has occurs
among its probes (receptor restraint, ligand restraint and membrane beads on the small complex; the two restraints on 1azp,
which has no bead); no refinement decides within MIN_GAP; every live swarm moves; the decoys are large enough for several parts,
more than four passes of 16 and a grown workspace.  These are conditions on the chosen inputs, not measurements: the seeds in
scorer_history.py were chosen until the references met all of them."""
import collections

import numpy as np
import pytest

import refine_reference as rr
import scorer_history as sh
from refine_cases import MIN_GAP

# the outputs that carry a call's information, by name; what a probe and a decoy share of them is compared
INFORMATIVE = ("energies", "counts", "energy_before", "energy_after", "swarm0/scoring", "swarm0/luciferin", "energy", "pairs",
               "rec/sums", "lig/sums")


@pytest.fixture(scope="module")
def world(orc, table, tmp_path_factory):
    return sh.World(orc, table, tmp_path_factory.mktemp("scorer_history"))


def carries_information(name, stale, mine):
    """The elements of a probe's expected output that say something: not the caller's own sentinel, and for a per-atom sum
    not the zero that both the probe and the decoy have for an atom without a partner."""
    if name == "energies":
        return mine != sh.SENTINEL
    if name == "counts":
        return mine != sh.COUNT_SENTINEL
    if name.endswith("/sums"):
        return (mine != 0.0) | (stale != 0.0)
    return np.ones(mine.shape, dtype=bool)


def stale_answer(world, probe, decoy):
    """The probe's expectation with every shared informative output replaced by the leading part of the decoy's."""
    want, left = world.expected(probe), world.expected(decoy)
    out = {k: np.array(v) for k, v in want.items() if not k.startswith("_")}
    for name in INFORMATIVE:
        if name in want and name in left:
            stale, mine = sh.leading(left[name], want[name])
            flat = out[name].reshape(-1)
            flat[:len(stale)] = stale
    return out


class Reports:
    """What held() asks of a scorer: the pair kernel's name (it chooses _against_oracle's measure)."""

    def __init__(self, handle):
        self.name = sh.HANDLES[handle][2]

    def kernel_info(self):
        return {"pair_kernel_name": self.name}


def as_answer(world, call, outputs):
    """{output name: array} in the shape World.run returns it, so that World.held can judge it without a library."""
    got = dict(outputs)
    if call.entry == "decompose":
        n = len(call.poses)
        got["_got"] = {key: {k: outputs["%s/%s" % (key, k)] for k in sh.SIDE_KEYS} for key in ("rec", "lig")}
        terms = [dict(w["terms"], reserved=0) for w in world.expected(call)["_restated"]]
        for i in range(n):
            terms[i]["energy"], terms[i]["pairs"] = outputs["energy"][i], int(outputs["pairs"][i])
        got["_terms"] = terms
    return got


@pytest.mark.parametrize("complex_", sh.COMPLEXES)
def test_a_probe_that_returned_what_a_decoy_left_would_fail(world, complex_):
    """Every (decoy X, probe Y) whose outputs share a name: the leading probe.size elements of the decoy's differ from the
    probe's in every element that carries information."""
    shared = 0
    for y in sh.ENTRIES:
        probe = world.expected(world.call(y, "probe", complex_))
        for x in sh.ENTRIES:
            decoy = world.expected(world.call(x, "decoy", complex_))
            for name in INFORMATIVE:
                if name in probe and name in decoy and probe[name].size and decoy[name].size:
                    stale, mine = sh.leading(decoy[name], probe[name])
                    tells = carries_information(name, stale, mine)
                    if not tells.any():         # (a one-pose decoy against a probe whose first row is masked out)
                        continue
                    assert np.all(stale[tells] != mine[tells]), (x, y, name)
                    shared += 1
    assert shared >= 20


@pytest.mark.parametrize("handle", sh.HANDLES)
def test_swapping_a_probes_expectation_for_a_decoys_leading_part_is_noticed(world, handle):
    """The check the GPU test applies (World.held), on the CPU: the expectation itself passes it, the expectation with the
    leading part of any decoy's in its place does not."""
    c = sh.HANDLES[handle][0]
    for y in sh.ENTRIES:
        probe = world.call(y, "probe", c)
        mine = {k: v for k, v in world.expected(probe).items() if not k.startswith("_")}
        world.held(handle, Reports(handle), probe, as_answer(world, probe, mine))
        if y == "zero_rows":
            continue
        for x in sh.ENTRIES:
            decoy = world.call(x, "decoy", c)
            if not any(n in mine and n in world.expected(decoy) and world.expected(decoy)[n].size for n in INFORMATIVE):
                continue
            with pytest.raises(AssertionError):
                world.held(handle, Reports(handle), probe, as_answer(world, probe, stale_answer(world, probe, decoy)))


@pytest.mark.parametrize("complex_", sh.COMPLEXES)
def test_the_far_pose_and_every_tail_term_occur_among_the_probes(world, complex_):
    cpu, L = world.cpu[complex_], world.pose_len[complex_]
    bare = 4.7 if world.small(complex_) else 0.0
    for entry in ("energy_batch", "device_mask", "device_counts"):
        call = world.call(entry, "probe", complex_)
        n = len(call.poses)
        assert 0 < n <= 9 and n % 8 != 0 and call.poses.shape[1] == L
        on = call.params["active"] == 1 if "active" in call.params else np.ones(n, dtype=bool)
        assert on.sum() >= n - 1 and (entry == "energy_batch" or not on.all())
        ex = [cpu.energy_ex_row(row) for row in call.poses]
        far = [i for i, row in enumerate(call.poses) if tuple(row[:3]) == sh.FAR_T]
        assert len(far) == 1 and on[far[0]]
        assert ex[far[0]][1][5] == 0 and ex[far[0]][0] == bare and world.expected(call)["energies"][far[0]] == bare
        for term in world.tail_terms(complex_):
            assert any(s[term] > 0 and on[i] for i, (_, s) in enumerate(ex)), (entry, term)
    assert world.tail_terms(complex_) == ((2, 3, 4) if world.small(complex_) else (2, 3))


@pytest.mark.parametrize("complex_", sh.COMPLEXES)
def test_every_decoy_is_larger_and_other_than_its_probe(world, complex_):
    L, small = world.pose_len[complex_], world.small(complex_)
    for entry in sh.ENTRIES:
        probe, decoy = world.call(entry, "probe", complex_), world.call(entry, "decoy", complex_)
        if entry in ("energy", "zero_rows"):        # one pose, or none: nothing to enlarge
            assert len(probe.poses) == len(decoy.poses) == (1 if entry == "energy" else 0)
        elif entry == "gso":
            assert probe.poses.shape == (1, 9, L) and decoy.poses.shape == (3, 24, L)
            assert (probe.params["steps"], decoy.params["steps"]) == (4, 5) and not set(probe.params["seeds"]) & set(decoy.params["seeds"])
        else:
            assert len(decoy.poses) > len(probe.poses) and decoy.poses.shape[1] == L + 2 and probe.poses.shape[1] == L
        if entry in ("energy_batch", "device_mask", "device_counts"):
            # several parts of 64 entries and, in passes of 16, more than four passes on two sets; 24 rows on 1azp
            assert len(decoy.poses) >= (65 if small else 20)
        if entry == "refine":
            assert all(probe.params[k] != decoy.params[k] for k in ("iterations", "steps", "max_halvings", "slice_poses"))
            trials = rr.trial_count(L)
            assert len(decoy.poses) * trials > max(len(world.call(e, "decoy", complex_).poses) for e in ("energy_batch", "device_mask")), "grows the workspace"
        if "active" in probe.params:
            assert not np.array_equal(probe.params["active"], decoy.params["active"][:len(probe.poses)])
        if L > 7 and entry in ("energy_batch", "energy", "device_mask", "device_counts", "decompose", "refine"):
            wild = np.abs(decoy.poses[:, 7:L]).max(axis=1)        # one row's amplitudes x 40
            assert (wild > 10.0 * np.median(wild)).sum() == 1 or len(wild) < 3 and wild.max() > 25.0, entry
    batch = world.call("energy_batch", "decoy", complex_)
    bad = batch.params["degenerate"]
    assert len(bad) == 2 and np.isnan(batch.poses[bad[0], 0]) and not batch.poses[bad[1], 3:7].any() and min(bad) >= 9
    if small:
        assert len(batch.poses) > 4 * 16 and -(-len(batch.poses) // 16) == 5, "bm16: five passes of 16"
        ex = [world.cpu[complex_].energy_ex_row(row[:L])[1] for row in batch.poses]
        assert sum(s[5] > 0 for s in ex) > 64, "tile pairs of more than 64 entries: several parts"


@pytest.mark.parametrize("complex_", sh.COMPLEXES)
def test_no_refinement_decides_within_the_gap(world, complex_):
    for kind in ("probe", "decoy", "flip-sliced", "flip-whole", "grow"):
        want = world.expected(world.call("refine", kind, complex_))
        assert want["_min_gap"] >= MIN_GAP, (kind, want["_min_gap"])
        assert want["accepted"].sum() > 0 and (want["history"] >= 0).any()
    grow, decoy = world.call("refine", "grow", complex_), world.call("refine", "decoy", complex_)
    assert grow.params["slice_poses"] == 0 and len(grow.poses) > 2 * len(decoy.poses), "more trial rows in one pass than anything before"
    a, b = (world.call("refine", k, complex_) for k in ("flip-sliced", "flip-whole"))
    assert a.params["slice_poses"] == 2 < len(a.poses) and b.params["slice_poses"] == 0


@pytest.mark.parametrize("complex_", sh.COMPLEXES)
def test_every_live_swarm_moves_and_the_still_one_does_not(world, complex_):
    for kind, live, still in (("probe", (0,), ()), ("probe2", (0,), ()), ("graph", (0,), ()), ("decoy", (0, 2), (1,))):
        call = world.call("gso", kind, complex_)
        steps = world.expected(call)["_steps"]
        assert len(steps) == call.params["steps"]
        for s in live:
            assert sum(int(st[s]["moved"].sum()) for st in steps[:4]) > 0, (kind, s)
            assert sum(int(st[s]["moved"].sum()) for st in steps[:2]) > 0, (kind, s, "before the other callers come in")
        for s in still:
            assert not any(st[s]["moved"].any() for st in steps) and np.array_equal(steps[-1][s]["poses"], call.poses[s])
    a, b = world.call("gso", "probe", complex_), world.call("gso", "probe2", complex_)
    assert a.params["seeds"][0] != b.params["seeds"][0] and not np.array_equal(a.poses, b.poses)


def test_the_histories_are_what_they_claim(world):
    for handle in sh.HANDLES:
        seen = collections.Counter()
        for x in sh.ENTRIES:
            row = world.pair_row(handle, x)
            assert [s.call.entry for s in row[::2]] == [x] * 8 and [s.call.kind for s in row[::2]] == ["decoy"] * 8
            assert [s.call.entry for s in row[1::2]] == list(sh.ENTRIES) and [s.call.kind for s in row[1::2]] == ["probe"] * 8
            assert all(s.expect == sh.OK and s.call.complex == sh.HANDLES[handle][0] for s in row)
            seen.update((a.call.entry, b.call.entry) for a, b in zip(row[::2], row[1::2]))
            bad = world.refusals(handle, x)
            hows = sh.REFUSALS[x]
            assert len(bad) == 8 * (len(hows) + 1)
            for k in range(8):
                block = bad[k * (len(hows) + 1):(k + 1) * (len(hows) + 1)]
                assert [s.expect for s in block] == list(hows) + [sh.OK] and block[-1].call is world.of(handle, sh.ENTRIES[k], "probe")
        assert len(seen) == 64 and set(seen.values()) == {1}
        assert [s.call.kind for s in world.soak(handle)] == ["decoy"] * 8
        assert [s.call.kind for s in world.growth(handle)] == ["probe"] * 8 + ["decoy"] * 8 + ["probe"] * 8
        flips = world.flip_history(handle)
        heads = flips[::9]
        assert len(flips) == 15 * 9 and all([s.call for s in flips[k * 9 + 1:k * 9 + 9]] == [s.call for s in world.probes(handle)] for k in range(15))
        assert [len(s.call.poses) for s in heads[:9]] == list(sh.FLIP_BATCHES)
        assert [(s.call.entry, len(s.call.poses)) for s in heads[9:13]] == [("device_counts", 9), ("device_mask", 65), ("device_counts", 65), ("device_mask", 9)]
        assert [s.call.params["slice_poses"] for s in heads[13:]] == [2, 0]
        for s in heads:
            assert world.expected(s.call) is not None
        assert [s.call.kind for s in world.between(handle)] == ["decoy"] * 8 + ["grow"]
        quiet = world.quiet_decoys(handle)
        grown = {e: len(world.of(handle, e, "decoy").poses) for e in ("energy_batch", "device_counts", "decompose")}
        assert [s.call.entry for s in quiet] == ["energy_batch", "device_counts", "decompose"]
        assert all(len(s.call.poses) <= 9 and len(s.call.poses) < grown[s.call.entry] for s in quiet), "no larger than the GSO's own batch, smaller than the soak's"
    assert sum(len(h) > 0 for h in sh.REFUSALS.values()) == 7
    both = world.two_handles()
    assert [h for h, _ in both] == ["bm", "bm-anm"] * 16 and both[0][1].call.complex == "rigid" and both[1][1].call.complex == "anm"
    assert world.build["rigid"][1:3] == world.build["anm"][1:3], "they share files"
    assert set(sh.GRAPH_HANDLES) == {"bm", "bm16", "dna"}
