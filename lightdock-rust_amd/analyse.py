"""Analysis of a finished run, as example/1czy/analysis.sh does it with LightDock's tools (lgd_cluster_bsas.py per swarm,
lgd_rank.py, lgd_top.py), with the posing and clustering of every swarm in ONE ld_complex_cluster call on the GPU.

    cd run_dir && python lightdock-rust_amd/analyse.py <setup.json> <step> [--swarms 0-9] [--top N] [--cutoff 4.0]

Reads swarm_<i>/gso_<step>.out and writes swarm_<i>/cluster.repr, rank_by_scoring.list and top/top_<k>.pdb.
Path rules as launch.py.  No per-glowworm PDB files are written.
"""
import os
import sys

import numpy as np

try:
    from .run_dir import argument_parser, build_complex, open_run, ranking, read_gso, swarm_list
except ImportError:  # run as a script
    from run_dir import argument_parser, build_complex, open_run, ranking, read_gso, swarm_list

RANK_HEADER = ("Swarm  Glowworm   Coordinates                                             RecID  LigID  Luciferin  Neigh   VR"
               "     RMSD    PDB             Clashes  Scoring\n")


def cluster_repr_lines(cluster_of, representatives, n_clusters, scoring):
    """lgd_cluster_bsas.py's cluster.repr of one swarm."""
    sizes = np.bincount(cluster_of, minlength=n_clusters)
    return ["%d:%d:%8.5f:%d:lightdock_%d.pdb\n" % (c, sizes[c], scoring[r], r, r) for c, r in enumerate(representatives[:n_clusters])]


def rank_by_scoring_text(entries):
    return RANK_HEADER + "".join(
        "%5d %6d %60s %6d %6d %11.5f %5d %7.3f %8.3f %16s %6d %8.3f\n"
        % (s, g, "(" + ", ".join("%.3f" % v for v in pose) + ")", c["rec_id"], c["lig_id"], c["luciferin"], c["neighbors"],
           c["vision_range"], -1.0, "lightdock_%d.pdb" % g, 0, c["scoring"]) for s, g, pose, c in entries)


def printed_pose(pose):
    """The pose as rank_by_scoring.list prints it (3 decimals), which is what lgd_top.py poses."""
    return np.array([float("%.3f" % v) for v in pose])


def main(argv=None):
    ap = argument_parser(every=False)
    ap.add_argument("--top", type=int, default=10, help="number of top_<k>.pdb files")
    ap.add_argument("--cutoff", type=float, default=4.0, help="BSAS RMSD cutoff (A)")
    args = ap.parse_args(argv)

    pkg, setup, sim = open_run(args.setup)
    cx = build_complex(pkg, setup, sim)

    swarms = swarm_list(args.swarms, setup)
    runs = [read_gso(os.path.join("swarm_%d" % s, "gso_%d.out" % args.step)) for s in swarms]
    if len({p.shape for p, _ in runs}) != 1 or runs[0][0].shape[1] < cx.pose_len:
        raise ValueError("every gso_%d.out must hold as many glowworms, of at least %d columns" % (args.step, cx.pose_len))
    scoring = np.stack([c["scoring"] for _, c in runs])
    res = cx.cluster(np.stack([p[:, :cx.pose_len] for p, _ in runs]), scoring, args.cutoff)
    for k, s in enumerate(swarms):
        with open(os.path.join("swarm_%d" % s, "cluster.repr"), "w") as f:
            f.writelines(cluster_repr_lines(res["cluster_of"][k], res["representatives"][k], int(res["n_clusters"][k]), scoring[k]))

    entries = ranking(swarms, args.step)
    with open("rank_by_scoring.list", "w") as f:
        f.write(rank_by_scoring_text(entries))
    top = entries[:max(0, args.top)]
    if top:
        os.makedirs("top", exist_ok=True)
    for k, (_, _, pose, _) in enumerate(top, 1):
        cx.write_pdb(printed_pose(pose)[:cx.pose_len], os.path.join("top", "top_%d.pdb" % k))
    print("%d swarms: %d clusters, %d top models" % (len(swarms), int(res["n_clusters"].sum()), len(top)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
