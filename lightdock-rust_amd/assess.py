"""Quality of the models of a run against a reference (bound) complex: fnat, i-RMSD, L-RMSD, DockQ and the CAPRI class of
every candidate, with ALL candidates in ONE ld_complex_assess call on the GPU.

    cd run_dir && python lightdock-rust_amd/assess.py <setup.json> <step> --reference-receptor REC.pdb --reference-ligand LIG.pdb
                                                       [--swarms 0-9] [--all] [--contact-cutoff 5.0] [--interface-cutoff 10.0]

Candidates as filter.py: the entries of rank_by_scoring.list as analyse.ranking() forms them, or with --all every glowworm
of every selected swarm, by scoring, highest first, ties in (swarm, glowworm) order.  The two reference files share one
frame, which need not be the run's; atoms are matched by chain, residue number, insertion code, residue name and atom name.
Writes assessment.list.  The rule is this project's (include/lightdock_hip.h, "Model quality"), modelled on CAPRI / DockQ;
no byte compatibility with any outside tool is claimed.  Path rules as launch.py.
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
    """entries: analyse.ranking() entries; the three measures per entry -> the text of assessment.list."""
    q = dockq(fnat, irmsd, lrmsd) if len(entries) else []
    return ASSESS_HEADER + "".join("%5d %9d %11.5f %7.3f %8.3f %8.3f %7.3f  %s\n" %
                                   (e[0], e[1], e[3]["scoring"], fnat[i], irmsd[i], lrmsd[i], q[i], capri_class(fnat[i], irmsd[i], lrmsd[i]))
                                   for i, e in enumerate(entries))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("setup")
    ap.add_argument("step", type=int)
    ap.add_argument("--reference-receptor", required=True, help="receptor of the bound complex (PDB)")
    ap.add_argument("--reference-ligand", required=True, help="ligand of the bound complex (PDB), in the same frame")
    ap.add_argument("--swarms", default=None, help="e.g. 0-9 or 0,3,7 (default: every swarm of setup.json)")
    ap.add_argument("--all", action="store_true", help="every glowworm, not only the ranked cluster representatives")
    ap.add_argument("--contact-cutoff", type=float, default=5.0, help="native contact distance (A)")
    ap.add_argument("--interface-cutoff", type=float, default=10.0, help="interface residue distance (A)")
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
    cx.set_reference(args.reference_receptor, args.reference_ligand, args.contact_cutoff, args.interface_cutoff)

    swarms = parse_swarm_list(args.swarms) if args.swarms else list(range(int(setup["swarms"])))
    entries = all_glowworms(swarms, args.step) if args.all else ranking(swarms, args.step)
    if any(len(e[2]) < cx.pose_len for e in entries):
        raise ValueError("gso_%d.out must hold poses of at least %d columns" % (args.step, cx.pose_len))
    poses = np.array([e[2][:cx.pose_len] for e in entries]).reshape(len(entries), cx.pose_len)
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
