"""Non-redundant ranked models of a run: BSAS over ONE list of candidates of all swarms, in one ld_complex_cluster_ranked
call on the GPU.  analyse.py clusters inside each swarm; neighbouring swarms converge on the same site, so its
rank_by_scoring.list holds the same model many times.  This step removes them and reports cluster populations.

    cd run_dir && python lightdock-rust_amd/cluster_run.py <setup.json> <step> [--swarms 0-9] [--all] [--cutoff 4.0]
                                                            [--atoms complex|ligand] [--top N]

Candidates, as filter.py chooses them: the entries of rank_by_scoring.list as run_dir.ranking() forms them from
swarm_<i>/cluster.repr and gso_<step>.out (the full-precision pose of the gso file); with --all every glowworm of every
selected swarm.  Both lists are by scoring, highest first, which is the order the clustering takes them in.  The measure:
the RMSD over the CA / P atoms of the whole complex (--atoms complex, lgd_cluster_bsas.py's) or of the ligand only
(--atoms ligand, which the receptor does not dilute), on the coordinates "%8.3f" prints, no superposition.
Writes clustered/rank_clustered.list (a line a cluster in creation order, best scoring first: cluster, size, and the swarm,
glowworm and scoring of its representative), clustered/members.list (cluster, swarm, glowworm, scoring of every candidate)
and, with --top N, clustered/cluster_<k>.pdb of the first N representatives.  No other file of the run is changed.  The rule
is this project's (include/lightdock_hip.h, "Clustering a ranked list").  Path rules as launch.py.
"""
import os
import sys

import numpy as np

try:
    from .run_dir import argument_parser, build_complex, candidates, open_run, pose_matrix, swarm_list
except ImportError:  # run as a script
    from run_dir import argument_parser, build_complex, candidates, open_run, pose_matrix, swarm_list

CLUSTERED_HEADER = "Cluster    Size  Swarm  Glowworm     Scoring\n"
MEMBERS_HEADER = "Cluster  Swarm  Glowworm     Scoring\n"


def rank_clustered_text(entries, cluster_of, representatives, n_clusters):
    """A line a cluster in creation order: cluster, size, swarm, glowworm and scoring of the representative."""
    sizes = np.bincount(np.asarray(cluster_of, dtype=np.int64), minlength=n_clusters)
    return CLUSTERED_HEADER + "".join("%7d %7d %6d %9d %11.5f\n" % (c, sizes[c], entries[r][0], entries[r][1], entries[r][3]["scoring"])
                                      for c, r in enumerate(representatives[:n_clusters]))


def members_text(entries, cluster_of):
    """A line a candidate, in the candidates' order: cluster, swarm, glowworm, scoring."""
    return MEMBERS_HEADER + "".join("%7d %6d %9d %11.5f\n" % (cluster_of[i], e[0], e[1], e[3]["scoring"]) for i, e in enumerate(entries))


def main(argv=None):
    ap = argument_parser()
    ap.add_argument("--cutoff", type=float, default=4.0, help="RMSD cutoff (A)")
    ap.add_argument("--atoms", choices=("complex", "ligand"), default="complex", help="the CA / P atoms measured")
    ap.add_argument("--top", type=int, default=0, help="number of cluster_<k>.pdb files")
    args = ap.parse_args(argv)

    pkg, setup, sim = open_run(args.setup)
    cx = build_complex(pkg, setup, sim)

    entries = candidates(swarm_list(args.swarms, setup), args.step, args.all)
    poses = pose_matrix(entries, args.step, cx.pose_len)
    scoring = np.array([e[3]["scoring"] for e in entries], dtype=np.float64)
    res = cx.cluster_ranked(poses, scoring, args.cutoff, args.atoms)
    cluster_of, reps, k = res["cluster_of"][0], res["representatives"][0], int(res["n_clusters"][0])

    os.makedirs("clustered", exist_ok=True)
    with open(os.path.join("clustered", "rank_clustered.list"), "w") as f:
        f.write(rank_clustered_text(entries, cluster_of, reps, k))
    with open(os.path.join("clustered", "members.list"), "w") as f:
        f.write(members_text(entries, cluster_of))
    top = reps[:min(k, max(0, args.top))]
    for c, r in enumerate(top, 1):
        cx.write_pdb(poses[r], os.path.join("clustered", "cluster_%d.pdb" % c))
    print("%d candidates: %d clusters, %d models written" % (len(entries), k, len(top)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
