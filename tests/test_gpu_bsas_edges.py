"""The clustering's RMSD test on the MI355X ON its threshold: ld_complex_cluster (complex_bsas, kernels/cluster.hip) and
ld_complex_cluster_ranked (ranked_pick, ranked_sweep, kernels/ranked.hip) against the exact integer oracle of tests/bsas_edges.py
at every case built there.  Every comparison is exact equality of all three outputs, the -1 padding included; no case is a tie
(tests/test_bsas_edges_cpu.py), so nothing is left out.

What a wrong kernel fails (each tried on an MI355X, the mutated library against this file).  An s_max one unit too small, or a
threshold off by any unit of S: test_threshold_pairs, every finite cutoff.  A last partial granule left out of the sum
(complex_bsas's b0 loop bounded by n_bb - n_bb % 32): the probes at floor(s*) + 1 whose deciding term sits in that granule join
the representative -- test_threshold_pairs at n = 1, 2, 31 over the complex, test_where_the_deciding_term_sits in every layout
but "one-granule", test_ranked_list_positions[complex], test_half_thousandths and test_range (a single atom IS the last granule).
thousandths() as a plain rint(x * 1000): test_half_thousandths, both complexes.  `S < s_max` for `S <= s_max` in ranked_pick: off a
tie s_max is never an integer (tests/bsas_edges.py, TIES), so no integer S can tell the two apart and nothing above notices;
test_at_a_tie_the_ranked_list_decides_as_the_per_swarm_kernel stands where s_max IS the integer S, and fails."""
import ctypes

import numpy as np
import pytest

import bsas_edges as be

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def complexes(pkg, tmp_path_factory):
    """spec -> Complex, each built once."""
    pkg.init(0)
    directory = str(tmp_path_factory.mktemp("bsas_edges"))
    made = {}

    def get(spec):
        if spec not in made:
            made[spec] = be.make_complex(pkg, spec, directory)
        return made[spec]

    return get


def check_row(got, k, want, where):
    """Row k of a call against the oracle's (cluster_of, representatives, ties): all three outputs, -1 after the last."""
    want_of, want_reps, ties = want
    assert ties == 0, where
    n = len(want_reps)
    assert int(got["n_clusters"][k]) == n, (where, int(got["n_clusters"][k]), n)
    assert np.array_equal(got["cluster_of"][k], want_of), (where, np.flatnonzero(got["cluster_of"][k] != np.array(want_of))[:8])
    assert list(got["representatives"][k][:n]) == list(want_reps), where
    assert np.all(got["representatives"][k][n:] == -1), where


def same_words(a, b):
    return all(np.array_equal(a[key], b[key]) for key in ("cluster_of", "representatives", "n_clusters"))


def run_case(cx, case, per_swarm=True):
    """cluster_ranked under every measure the case is built for; under the complex's, cluster on the list as one swarm (the same
    words as cluster_ranked) and on case.swarms in one call."""
    assert cx.num_atoms(2) == case.spec.n_rec_bb + case.spec.n_lig_bb
    for measure, want in case.expected.items():
        ranked = cx.cluster_ranked(case.poses, case.scoring, case.cutoff, measure)
        check_row(ranked, 0, want, (case.name, "ranked", measure))
        if measure == "complex" and per_swarm:
            one = cx.cluster(case.poses[None], case.scoring[None], case.cutoff)
            check_row(one, 0, want, (case.name, "one swarm"))
            assert same_words(ranked, one), case.name
            if case.swarms is not None:
                many = cx.cluster(case.poses[case.swarms], case.scoring[case.swarms], case.cutoff)
                for k, want_k in enumerate(be.swarm_expected(case)):
                    check_row(many, k, want_k, (case.name, "swarm", k))


@pytest.mark.parametrize("n,measure", be.THRESHOLD_GROUPS)
def test_threshold_pairs(complexes, n, measure):
    """A representative and probes at S = floor(s*) - 1 ... floor(s*) + 2 from it, at every cutoff of bsas_edges.CUTOFFS."""
    for case in be.threshold_cases(n, measure):
        run_case(complexes(case.spec), case)


@pytest.mark.parametrize("layout,measure", be.WHERE_GROUPS)
def test_where_the_deciding_term_sits(complexes, layout, measure):
    """S = floor(s*) and floor(s*) + 1 whole in each mover and split over each pair of movers; inside the first 64 candidates
    (ranked_pick, complex_bsas) and behind them (ranked_sweep, its first granule in registers and the walk beyond it)."""
    for fillers in be.WHERE_FILLERS:
        case = be.where_case(layout, measure, fillers)
        run_case(complexes(case.spec), case)


@pytest.mark.parametrize("measure", be.MEASURES)
def test_ranked_list_positions(complexes, measure):
    """The probes at sorted positions 64, 255, 256 and 300 behind far-away fillers, and a probe between two leaders that joins
    the second (floor(s*) + 1 from the first) or the first (floor(s*) from both); the lists are handed over shuffled."""
    cases = [be.position_case(measure, pos) for pos in be.POSITIONS]
    cases += [be.two_leader_case(measure, joins, fillers) for joins in (1, 2) for fillers in (0, 70)]
    for case in cases:
        run_case(complexes(case.spec), case)


@pytest.mark.parametrize("which", sorted(be.HALF_SPECS))
def test_half_thousandths(complexes, which):
    """500 swarms of a pose at the double nearest (k + 0.5) / 1000 with the poses at k / 1000 and (k + 1) / 1000, cutoff 0.0: the
    grouping is the decimal expansion's; and the 1500 poses as one list."""
    case = be.half_case(which)
    run_case(complexes(case.spec), case)


@pytest.mark.parametrize("which", sorted(be.HALF_SPECS))
def test_range(pkg, complexes, which):
    """Differences near 2^32 thousandths; a thousandth at exactly 2 147 483 647 is accepted, one more is refused with status -1
    and the outputs are left untouched."""
    for case in be.range_cases(which):
        run_case(complexes(case.spec), case)
    spec = be.HALF_SPECS[which]
    cx, lib = complexes(spec), pkg.load_library()
    poses = np.ascontiguousarray(np.stack([be.pose_row(spec), be.refused_row(which)]))
    scoring = np.array([1.0, 0.0])
    stride = poses.shape[1]

    def outputs():
        return np.full(2, -7, dtype=np.int32), np.full(2, -7, dtype=np.int32), np.full(1, 12345, dtype=np.uint32)

    def untouched(status, cluster_of, reps, count):
        assert status == -1 and "beyond" in lib.ld_last_error().decode()
        assert np.all(cluster_of == -7) and np.all(reps == -7) and count[0] == 12345

    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    cluster_of, reps, count = outputs()
    untouched(lib.ld_complex_cluster(cx._h, 1, 2, ptr(poses), stride, ptr(scoring), ctypes.c_double(4.0), ptr(cluster_of), ptr(reps),
                                     ptr(count)), cluster_of, reps, count)
    for atoms in range(len(be.half_case(which).expected)):
        cluster_of, reps, count = outputs()
        untouched(lib.ld_complex_cluster_ranked(cx._h, 2, ptr(poses), stride, ptr(scoring), ctypes.c_double(4.0), atoms, ptr(cluster_of),
                                                ptr(reps), ptr(count)), cluster_of, reps, count)
    with pytest.raises(pkg.LightdockError):
        cx.cluster(poses[None], scoring[None], 4.0)
    # and the complex still serves
    assert int(cx.cluster_ranked(poses[:1], scoring[:1], 4.0)["n_clusters"][0]) == 1


def test_at_a_tie_the_ranked_list_decides_as_the_per_swarm_kernel(complexes):
    """400 S == n (2K + 1)^2: the float path decides, and both calls evaluate the same one -- complex_bsas directly, the ranked
    kernels through s_max, which at these ties is the integer S itself.  No oracle: the two calls against each other."""
    for spec, poses, scoring, cutoff, S in be.tie_cases():
        cx = complexes(spec)
        ranked = cx.cluster_ranked(poses, scoring, cutoff, "complex")
        one = cx.cluster(poses[None], scoring[None], cutoff)
        print("n %d, cutoff %.4f, S %d: per swarm %d clusters, ranked %d, the f64 expression on the host %d"
              % (spec.n_rec_bb + spec.n_lig_bb, cutoff, S, int(one["n_clusters"][0]), int(ranked["n_clusters"][0]),
                 2 - be.float_path(S, spec.n_rec_bb + spec.n_lig_bb, cutoff)))
        assert same_words(ranked, one), (spec, cutoff)
