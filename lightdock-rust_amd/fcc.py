"""Models of a run grouped by what their interface is made of: clustering by the fraction of common contacts (FCC) over ONE
list of candidates of all swarms, in one ld_complex_cluster_fcc call on the GPU, with a CONSRANK-style consensus score.
cluster_run.py measures how far the posed coordinates of two models are apart; this step compares the residue pairs in
contact, so the receptor does not dilute the measure and a cluster's population does not depend on the order of the list.

    cd run_dir && python lightdock-rust_amd/fcc.py <setup.json> <step> [--swarms 0-9] [--all] [--cutoff 5.0] [--threshold 0.6]
                                                    [--min-size 1] [--top N]

Candidates, as cluster_run.py chooses them: the entries of rank_by_scoring.list as run_dir.ranking() forms them, or with
--all every glowworm of every selected swarm; both by scoring, highest first.  A model's set: the (receptor residue,
ligand residue) pairs with two atoms within --cutoff on the coordinates "%8.3f" prints.  Two models are neighbours when the
pairs they share are at least --threshold of the larger set; the model with most neighbours and its neighbours form the
next cluster, until the largest would be below --min-size (the rest gets cluster -1).
Writes fcc/rank_fcc.list (a line a cluster in creation order: cluster, size, the swarm, glowworm and scoring of its centre,
the best scoring among its members), fcc/members.list (a line a candidate: cluster, swarm, glowworm, scoring, set size and the
consensus fraction, how often on average its pairs recur over the list) and, with --top N, fcc/cluster_<k>.pdb of the first
N centres.  No other file of the run is changed.  The rule is this project's (include/lightdock_hip.h, "Clustering by
common contacts").  Path rules as launch.py.
"""
import os
import sys

import numpy as np

try:
    from .run_dir import argument_parser, build_complex, candidates, open_run, pose_matrix, swarm_list
except ImportError:  # run as a script
    from run_dir import argument_parser, build_complex, candidates, open_run, pose_matrix, swarm_list

RANK_HEADER = "Cluster    Size  Swarm  Glowworm     Scoring        Best\n"
MEMBERS_HEADER = "Cluster  Swarm  Glowworm     Scoring    Pairs  Consensus\n"


def rank_fcc_text(entries, cluster_of, centres, n_clusters):
    """A line a cluster in creation order: cluster, size, swarm, glowworm and scoring of the centre, best scoring inside."""
    cluster_of = np.asarray(cluster_of, dtype=np.int64)
    scoring = np.array([e[3]["scoring"] for e in entries], dtype=np.float64)
    lines = []
    for c, r in enumerate(centres[:n_clusters]):
        members = cluster_of == c
        lines.append("%7d %7d %6d %9d %11.5f %11.5f\n" % (c, members.sum(), entries[r][0], entries[r][1], scoring[r], scoring[members].max()))
    return RANK_HEADER + "".join(lines)


def members_text(entries, cluster_of, set_sizes, fraction):
    """A line a candidate, in the candidates' order: cluster, swarm, glowworm, scoring, set size, consensus fraction."""
    return MEMBERS_HEADER + "".join("%7d %6d %9d %11.5f %8d %10.4f\n" % (cluster_of[i], e[0], e[1], e[3]["scoring"], set_sizes[i], fraction[i])
                                    for i, e in enumerate(entries))


def main(argv=None):
    ap = argument_parser()
    ap.add_argument("--cutoff", type=float, default=5.0, help="contact cutoff (A)")
    ap.add_argument("--threshold", type=float, default=0.6, help="fraction of the larger set two neighbours share")
    ap.add_argument("--min-size", type=int, default=1, help="smallest cluster kept")
    ap.add_argument("--top", type=int, default=0, help="number of cluster_<k>.pdb files")
    args = ap.parse_args(argv)

    pkg, setup, sim = open_run(args.setup)
    cx = build_complex(pkg, setup, sim)

    entries = candidates(swarm_list(args.swarms, setup), args.step, args.all)
    poses = pose_matrix(entries, args.step, cx.pose_len)
    scoring = np.array([e[3]["scoring"] for e in entries], dtype=np.float64)
    res = cx.cluster_fcc(poses, scoring, args.cutoff, args.threshold, args.min_size)
    k = res["n_clusters"]

    os.makedirs("fcc", exist_ok=True)
    with open(os.path.join("fcc", "rank_fcc.list"), "w") as f:
        f.write(rank_fcc_text(entries, res["cluster_of"], res["centres"], k))
    with open(os.path.join("fcc", "members.list"), "w") as f:
        f.write(members_text(entries, res["cluster_of"], res["set_sizes"], pkg.fcc_consensus_fraction(res["consensus"], res["set_sizes"])))
    top = res["centres"][:min(k, max(0, args.top))]
    for c, r in enumerate(top, 1):
        cx.write_pdb(poses[r], os.path.join("fcc", "cluster_%d.pdb" % c))
    print("%d candidates: %d clusters, %d models written" % (len(entries), k, len(top)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
