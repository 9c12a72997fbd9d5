"""Clustering by common contacts (ld_complex_pair_contacts, ld_fcc_cluster, lightdock-rust_amd/fcc.py) on
the CPU: the int64 numpy restatement of tests/fcc_reference.py (the checker the GPU tests use) on hand-made sets whose
clusters the rule pins, pinned on counts of the committed runs, and fcc.py's two text writers on hand-made arrays."""
import numpy as np

import fcc_reference as ref
from test_analysis_cpu import tool_module


def clusters(sets, scoring, threshold=0.6, min_size=1):
    offsets, keys = ref.to_csr(sets)
    return ref.cluster(offsets, keys, scoring, threshold, min_size)


SETS = [[1, 2, 3, 4], [1, 2, 3, 5], [1, 2, 3, 6], [], [4000000000, 4000000001], [4000000000, 4000000001], [77]]


def test_ties_go_to_the_larger_scoring_then_to_the_smaller_index():
    flat = clusters(SETS, np.zeros(7))
    assert flat["n_clusters"] == 4
    assert list(flat["cluster_of"]) == [0, 0, 0, 2, 1, 1, 3] and list(flat["centres"]) == [0, 4, 3, 6, -1, -1, -1]
    scored = clusters(SETS, [0.0, 2.0, 1.0, 9.0, -1.0, 5.0, 0.5])
    assert list(scored["cluster_of"]) == [0, 0, 0, 2, 1, 1, 3] and list(scored["centres"]) == [1, 5, 3, 6, -1, -1, -1]
    assert list(flat["consensus"]) == [10, 10, 10, 0, 4, 4, 1] and list(flat["set_sizes"]) == [4, 4, 4, 0, 2, 2, 1]
    assert list(ref.consensus_fraction(flat["consensus"], flat["set_sizes"])) == [10 / 28.0] * 3 + [0.0, 2 / 7.0, 2 / 7.0, 1 / 7.0]


def test_an_empty_set_has_no_neighbours_even_at_the_lowest_threshold():
    got = clusters([[], [], [5], [5, 6]], np.zeros(4), threshold=0.001)
    assert list(got["cluster_of"]) == [1, 2, 0, 0] and list(got["centres"]) == [2, 0, 1, -1]
    c = ref.common(*ref.to_csr([[], [], [5], [5, 6]]))
    assert c.tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 1, 1], [0, 0, 1, 2]]
    assert not ref.neighbours(c, np.array([0, 0, 1, 2]), 1)[:2].any()


def test_min_size_leaves_the_remainder_unclustered():
    scoring = [0.0, 2.0, 1.0, 9.0, -1.0, 5.0, 0.5]
    two = clusters(SETS, scoring, min_size=2)
    assert two["n_clusters"] == 2 and list(two["cluster_of"]) == [0, 0, 0, -1, 1, 1, -1] and list(two["centres"]) == [1, 5] + [-1] * 5
    three = clusters(SETS, scoring, min_size=3)
    assert three["n_clusters"] == 1 and list(three["cluster_of"]) == [0, 0, 0, -1, -1, -1, -1]
    none = clusters(SETS, scoring, min_size=8)
    assert none["n_clusters"] == 0 and (none["cluster_of"] == -1).all() and (none["centres"] == -1).all()


def test_a_pair_exactly_on_the_threshold_and_one_key_short_of_it():
    on = clusters([[1, 2, 3, 4, 5], [3, 4, 5, 8, 9]], [0.0, 1.0])                 # 1000 * 3 == 600 * 5
    assert on["n_clusters"] == 1 and list(on["cluster_of"]) == [0, 0] and list(on["centres"]) == [1, -1]
    short = clusters([[1, 2, 3, 4, 5], [3, 4, 5, 8, 9, 10]], [0.0, 1.0])          # 3000 < 600 * 6
    assert short["n_clusters"] == 2 and list(short["cluster_of"]) == [1, 0] and list(short["centres"]) == [1, 0]
    assert ref.threshold_thousandths(0.6) == 600 and ref.threshold_thousandths(0.001) == 1 and ref.threshold_thousandths(1.0) == 1000
    assert clusters(SETS, np.zeros(7), threshold=0.75)["n_clusters"] == 4 and clusters(SETS, np.zeros(7), threshold=0.751)["n_clusters"] == 6


def sizes_of(res):
    done = res["cluster_of"] >= 0
    return np.bincount(res["cluster_of"][done], minlength=res["n_clusters"])


def test_the_committed_1czy_run():
    poses, scoring, entries, offsets, keys, rs = ref.run_sets("1czy", 10)
    sizes = np.diff(offsets)
    assert (len(poses), sizes.min(), int(np.median(sizes)), sizes.max(), len(np.unique(keys))) == (2000, 2, 15, 81, 644)
    largest = {}
    for threshold, count in ((0.5, 79), (0.6, 95), (0.75, 112)):
        res = ref.cluster(offsets, keys, scoring, threshold, 1)
        assert res["n_clusters"] == count and (res["cluster_of"] >= 0).all()
        counts = sizes_of(res)
        assert counts.sum() == 2000 and (np.diff(counts) <= 0).all()
        assert (res["centres"][:count] >= 0).all() and (res["centres"][count:] == -1).all()
        assert list(res["cluster_of"][res["centres"][:count]]) == list(range(count))
        largest[threshold] = int(counts[0])
    assert largest == {0.5: 169, 0.6: 137, 0.75: 127}
    kept = ref.cluster(offsets, keys, scoring, 0.6, 4)
    assert kept["n_clusters"] == 77 and int((kept["cluster_of"] < 0).sum()) == 23 and (np.diff(sizes_of(kept)) <= 0).all()
    assert list(res["consensus"][:3]) == [3370, 3867, 3664]
    # the projection of the sets is the contacts' rows
    rec, lig = ref.projection(offsets[:41], keys[:offsets[40]], len(rs.rec_ids), len(rs.lig_ids))
    want_rec, want_lig = rs.batch(poses[:40])
    assert np.array_equal(rec, want_rec) and np.array_equal(lig, want_lig) and rec.any()


def test_the_committed_1azp_swarm():
    poses, scoring, entries, offsets, keys, rs = ref.run_sets("1azp", 1)
    sizes = np.diff(offsets)
    assert (len(poses), sizes.min(), int(np.median(sizes)), sizes.max(), len(np.unique(keys))) == (200, 5, 22, 47, 144)
    for threshold, largest in ((0.5, 44), (0.6, 39), (0.75, 39)):
        res = ref.cluster(offsets, keys, scoring, threshold, 1)
        counts = sizes_of(res)
        assert res["n_clusters"] == 11 and counts[0] == largest and (np.diff(counts) <= 0).all()
    rec, lig = ref.projection(offsets, keys, len(rs.rec_ids), len(rs.lig_ids))
    want_rec, want_lig = rs.batch(poses[:, :27])
    assert np.array_equal(rec, want_rec) and np.array_equal(lig, want_lig)


def test_the_text_of_rank_fcc_list_and_members_list():
    tool = tool_module("fcc")
    entries = [(0, 1, None, {"scoring": 7.25}), (3, 0, None, {"scoring": 7.25}), (0, 0, None, {"scoring": 1.5}),
               (0, 2, None, {"scoring": 1.5}), (3, 2, None, {"scoring": -2.0})]
    cluster_of, centres = np.array([1, 0, 0, -1, 0]), np.array([2, 0, -1, -1, -1])
    assert tool.rank_fcc_text(entries, cluster_of, centres, 2) == (
        "Cluster    Size  Swarm  Glowworm     Scoring        Best\n"
        "      0       3      0         0     1.50000     7.25000\n"
        "      1       1      0         1     7.25000     7.25000\n")
    assert tool.rank_fcc_text(entries, np.full(5, -1), np.full(5, -1), 0) == tool.RANK_HEADER
    assert tool.members_text(entries, cluster_of, np.array([12, 3, 0, 81, 7]), np.array([0.51236, 1.0, 0.0, 0.00004, 0.25])) == (
        "Cluster  Swarm  Glowworm     Scoring    Pairs  Consensus\n"
        "      1      0         1     7.25000       12     0.5124\n"
        "      0      3         0     7.25000        3     1.0000\n"
        "      0      0         0     1.50000        0     0.0000\n"
        "     -1      0         2     1.50000       81     0.0000\n"
        "      0      3         2    -2.00000        7     0.2500\n")
