"""Reading a finished run, for the post-run tools (analyse.py, filter.py, assess.py, cluster_run.py, decompose.py): the gso
files and the candidate lists made of them, and what every tool's main() does before its one GPU call -- the common
arguments, opening the run of a setup.json, the Complex of its two PDB files, the swarm list, the pose matrix.  Plain
Python: the library is imported by open_run() only.  Path rules as launch.py.
"""
import argparse
import json
import os
import sys

import numpy as np

try:
    from .launch import build_scorer, load_nmodes, parse_swarm_list  # noqa: F401
except ImportError:  # run as a script
    from launch import build_scorer, load_nmodes, parse_swarm_list  # noqa: F401

COLUMNS = (("rec_id", int), ("lig_id", int), ("luciferin", float), ("neighbors", int), ("vision_range", float), ("scoring", float))


def read_gso(path):
    """gso_<step>.out -> (poses (G, columns), dict of the per-glowworm columns)."""
    poses, cols = [], {k: [] for k, _ in COLUMNS}
    for line in open(path):
        if line.startswith("("):
            inner, rest = line[1:].split(")", 1)
            poses.append([float(v) for v in inner.split(",")])
            for (k, kind), v in zip(COLUMNS, rest.split()):
                cols[k].append(kind(v))
    return np.array(poses), {k: np.array(v) for k, v in cols.items()}


def ranking(swarms, step, base="."):
    """lgd_rank.py: the representatives of every swarm (swarm, then cluster order) from cluster.repr, sorted by scoring,
    highest first (stable).  Entries: (swarm, glowworm, pose row, columns)."""
    entries = []
    for s in swarms:
        d = os.path.join(base, "swarm_%d" % s)
        poses, cols = read_gso(os.path.join(d, "gso_%d.out" % step))
        for line in filter(str.strip, open(os.path.join(d, "cluster.repr"))):
            g = int(line.split(":")[3])
            entries.append((s, g, poses[g], {k: v[g] for k, v in cols.items()}))
    return sorted(entries, key=lambda e: e[3]["scoring"], reverse=True)


def all_glowworms(swarms, step, base="."):
    """Every glowworm of every swarm as ranking() entries, by scoring, highest first, ties in (swarm, glowworm) order."""
    entries = []
    for s in swarms:
        poses, cols = read_gso(os.path.join(base, "swarm_%d" % s, "gso_%d.out" % step))
        entries += [(s, g, poses[g], {k: v[g] for k, v in cols.items()}) for g in range(len(poses))]
    return sorted(entries, key=lambda e: (-e[3]["scoring"], e[0], e[1]))


def candidates(swarms, step, every=False, base="."):
    """ranking() entries (swarm, glowworm, pose row, columns): the ranked representatives, or every glowworm."""
    return all_glowworms(swarms, step, base) if every else ranking(swarms, step, base)


def argument_parser(every=True):
    """The arguments every tool takes: setup, step, --swarms and, where the tool chooses candidates, --all."""
    ap = argparse.ArgumentParser()
    ap.add_argument("setup")
    ap.add_argument("step", type=int)
    ap.add_argument("--swarms", default=None, help="e.g. 0-9 or 0,3,7 (default: every swarm of setup.json)")
    if every:
        ap.add_argument("--all", action="store_true", help="every glowworm, not only the ranked cluster representatives")
    return ap


def open_run(setup_path):
    """setup.json's path -> (the package with the library initialised, the setup, the directory of the setup file)."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as ge
    pkg = ge.package()
    pkg.init(-1)
    return pkg, json.load(open(setup_path)), os.path.dirname(os.path.abspath(setup_path))


def build_complex(pkg, setup, sim):
    """The Complex of a run: the PDB files next to setup.json, the modes of the sides that setup.json flexes."""
    kw = {}
    for side in ("rec", "lig"):
        kw[side + "_num_anm"] = n = int(setup["anm_" + side]) if setup["use_anm"] else 0
        if n > 0:
            kw[side + "_nmodes"] = load_nmodes(side, sim)
    return pkg.Complex(os.path.join(sim, "lightdock_" + setup["receptor_pdb"]), os.path.join(sim, "lightdock_" + setup["ligand_pdb"]), **kw)


def swarm_list(text, setup):
    """--swarms, or every swarm of setup.json."""
    return parse_swarm_list(text) if text else list(range(int(setup["swarms"])))


def pose_matrix(entries, step, pose_len):
    """The first pose_len columns of every entry's pose row, (n, pose_len)."""
    if any(len(e[2]) < pose_len for e in entries):
        raise ValueError("gso_%d.out must hold poses of at least %d columns" % (step, pose_len))
    return np.array([e[2][:pose_len] for e in entries]).reshape(len(entries), pose_len)
