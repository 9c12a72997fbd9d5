"""Quality of the models of a run against a reference (bound) complex: fnat, i-RMSD, L-RMSD, DockQ and the CAPRI class of
every candidate, with ALL candidates in ONE ld_complex_assess call on the GPU.

    cd run_dir && python lightdock-rust_amd/assess.py <setup.json> <step> --reference-receptor REC.pdb --reference-ligand LIG.pdb
                                                       [--swarms 0-9] [--all] [--contact-cutoff 5.0] [--interface-cutoff 10.0]

Candidates as filter.py: the entries of rank_by_scoring.list as run_dir.ranking() forms them, or with --all every glowworm
of every selected swarm, by scoring, highest first, ties in (swarm, glowworm) order.  The two reference files share one
frame, which need not be the run's; atoms are matched by chain, residue number, insertion code, residue name and atom name.
Writes assessment.list.  The rule is this project's (include/lightdock_hip.h, "Model quality"), modelled on CAPRI / DockQ;
no byte compatibility with any outside tool is claimed.  Path rules as launch.py.
"""
import sys

import numpy as np

try:
    from .run_dir import argument_parser, build_complex, candidates, open_run, pose_matrix, swarm_list
except ImportError:  # run as a script
    from run_dir import argument_parser, build_complex, candidates, open_run, pose_matrix, swarm_list

ASSESS_HEADER = "Swarm  Glowworm     Scoring    fnat    iRMSD    LRMSD   DockQ  CAPRI\n"


def dockq(fnat, irmsd, lrmsd):
    """(fnat + 1 / (1 + (iRMSD / 1.5)^2) + 1 / (1 + (LRMSD / 8.5)^2)) / 3, elementwise."""
    fnat, irmsd, lrmsd = (np.asarray(v, dtype=np.float64) for v in (fnat, irmsd, lrmsd))
    return (fnat + 1.0 / (1.0 + (irmsd / 1.5) ** 2) + 1.0 / (1.0 + (lrmsd / 8.5) ** 2)) / 3.0


def capri_class(fnat, irmsd, lrmsd):
    """The CAPRI class of one model, best class first."""
    if fnat >= 0.5 and (lrmsd <= 1.0 or irmsd <= 1.0):
        return "high"
    if fnat >= 0.3 and (lrmsd <= 5.0 or irmsd <= 2.0):
        return "medium"
    if fnat >= 0.1 and (lrmsd <= 10.0 or irmsd <= 4.0):
        return "acceptable"
    return "incorrect"


def assessment_text(entries, fnat, irmsd, lrmsd):
    """entries: run_dir.ranking() entries; the three measures per entry -> the text of assessment.list."""
    q = dockq(fnat, irmsd, lrmsd) if len(entries) else []
    return ASSESS_HEADER + "".join("%5d %9d %11.5f %7.3f %8.3f %8.3f %7.3f  %s\n" %
                                   (e[0], e[1], e[3]["scoring"], fnat[i], irmsd[i], lrmsd[i], q[i], capri_class(fnat[i], irmsd[i], lrmsd[i]))
                                   for i, e in enumerate(entries))


def main(argv=None):
    ap = argument_parser()
    ap.add_argument("--reference-receptor", required=True, help="receptor of the bound complex (PDB)")
    ap.add_argument("--reference-ligand", required=True, help="ligand of the bound complex (PDB), in the same frame")
    ap.add_argument("--contact-cutoff", type=float, default=5.0, help="native contact distance (A)")
    ap.add_argument("--interface-cutoff", type=float, default=10.0, help="interface residue distance (A)")
    args = ap.parse_args(argv)

    pkg, setup, sim = open_run(args.setup)
    cx = build_complex(pkg, setup, sim)
    cx.set_reference(args.reference_receptor, args.reference_ligand, args.contact_cutoff, args.interface_cutoff)

    entries = candidates(swarm_list(args.swarms, setup), args.step, args.all)
    poses = pose_matrix(entries, args.step, cx.pose_len)
    got = cx.assess(poses)
    with open("assessment.list", "w") as f:
        f.write(assessment_text(entries, got["fnat"], got["irmsd"], got["lrmsd"]))
    classes = [capri_class(*v) for v in zip(got["fnat"], got["irmsd"], got["lrmsd"])]
    counts = cx.reference_counts()
    print("%d models against %d native pairs: %s" % (len(entries), counts["native_pairs"],
                                                    ", ".join("%d %s" % (classes.count(c), c) for c in ("high", "medium", "acceptable", "incorrect"))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
