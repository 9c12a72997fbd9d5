"""Non-redundant ranked models of a run: BSAS over ONE list of candidates of all swarms, in one ld_complex_cluster_ranked
call on the GPU.  analyse.py clusters inside each swarm; neighbouring swarms converge on the same site, so its
rank_by_scoring.list holds the same model many times.  This step removes them and reports cluster populations.

    cd run_dir && python lightdock-rust_amd/cluster_run.py <setup.json> <step> [--swarms 0-9] [--all] [--cutoff 4.0]
                                                            [--atoms complex|ligand] [--top N]

Candidates, as filter.py chooses them: the entries of rank_by_scoring.list as analyse.ranking() forms them from
swarm_<i>/cluster.repr and gso_<step>.out (the full-precision pose of the gso file); with --all every glowworm of every
selected swarm.  Both lists are by scoring, highest first, which is the order the clustering takes them in.  The measure:
the RMSD over the CA / P atoms of the whole complex (--atoms complex, lgd_cluster_bsas.py's) or of the ligand only
(--atoms ligand, which the receptor does not dilute), on the coordinates "%8.3f" prints, no superposition.
Writes clustered/rank_clustered.list (a line a cluster in creation order, best scoring first: cluster, size, and the swarm,
glowworm and scoring of its representative), clustered/members.list (cluster, swarm, glowworm, scoring of every candidate)
and, with --top N, clustered/cluster_<k>.pdb of the first N representatives.  No other file of the run is changed.  The rule
is this project's (include/lightdock_hip.h, "Clustering a ranked list").  Path rules as launch.py.
"""
import argparse
import json
import os
import sys

import numpy as np

try:
    from .analyse import ranking
    from .filter import all_glowworms
    from .launch import load_nmodes, parse_swarm_list
except ImportError:  # run as a script
    from analyse import ranking
    from filter import all_glowworms
    from launch import load_nmodes, parse_swarm_list

CLUSTERED_HEADER = "Cluster    Size  Swarm  Glowworm     Scoring\n"
MEMBERS_HEADER = "Cluster  Swarm  Glowworm     Scoring\n"


def candidates(swarms, step, every=False, base="."):
    """analyse.ranking() entries (swarm, glowworm, pose row, columns): the ranked representatives, or every glowworm."""
    return all_glowworms(swarms, step, base) if every else ranking(swarms, step, base)


def rank_clustered_text(entries, cluster_of, representatives, n_clusters):
    """A line a cluster in creation order: cluster, size, swarm, glowworm and scoring of the representative."""
    sizes = np.bincount(np.asarray(cluster_of, dtype=np.int64), minlength=n_clusters)
    return CLUSTERED_HEADER + "".join("%7d %7d %6d %9d %11.5f\n" % (c, sizes[c], entries[r][0], entries[r][1], entries[r][3]["scoring"])
                                      for c, r in enumerate(representatives[:n_clusters]))


def members_text(entries, cluster_of):
    """A line a candidate, in the candidates' order: cluster, swarm, glowworm, scoring."""
    return MEMBERS_HEADER + "".join("%7d %6d %9d %11.5f\n" % (cluster_of[i], e[0], e[1], e[3]["scoring"]) for i, e in enumerate(entries))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("setup")
    ap.add_argument("step", type=int)
    ap.add_argument("--swarms", default=None, help="e.g. 0-9 or 0,3,7 (default: every swarm of setup.json)")
    ap.add_argument("--all", action="store_true", help="every glowworm, not only the ranked cluster representatives")
    ap.add_argument("--cutoff", type=float, default=4.0, help="RMSD cutoff (A)")
    ap.add_argument("--atoms", choices=("complex", "ligand"), default="complex", help="the CA / P atoms measured")
    ap.add_argument("--top", type=int, default=0, help="number of cluster_<k>.pdb files")
    args = ap.parse_args(argv)

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as ge
    pkg = ge.package()
    pkg.init(-1)
    setup = json.load(open(args.setup))
    sim = os.path.dirname(os.path.abspath(args.setup))
    kw = {}
    for side in ("rec", "lig"):
        kw[side + "_num_anm"] = n = int(setup["anm_" + side]) if setup["use_anm"] else 0
        if n > 0:
            kw[side + "_nmodes"] = load_nmodes(side, sim)
    cx = pkg.Complex(os.path.join(sim, "lightdock_" + setup["receptor_pdb"]), os.path.join(sim, "lightdock_" + setup["ligand_pdb"]), **kw)

    swarms = parse_swarm_list(args.swarms) if args.swarms else list(range(int(setup["swarms"])))
    entries = candidates(swarms, args.step, args.all)
    if any(len(e[2]) < cx.pose_len for e in entries):
        raise ValueError("gso_%d.out must hold poses of at least %d columns" % (args.step, cx.pose_len))
    poses = np.array([e[2][:cx.pose_len] for e in entries]).reshape(len(entries), cx.pose_len)
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
