"""How much surface every model of a run buries, and on which residues, with ALL candidates in ONE ld_complex_sasa call on
the GPU (include/lightdock_hip.h, "Solvent-accessible surface": Shrake-Rupley on the integer thousandths "%8.3f" prints,
128 points an atom, hydrogens and membrane beads left out).

    cd run_dir && python lightdock-rust_amd/interface.py <setup.json> <step> [--swarms 0-9] [--all] [--probe 1.4] [--top N]

Candidates as filter.py: the entries run_dir.ranking() forms from swarm_<i>/cluster.repr and gso_<step>.out, or with --all
every glowworm of every selected swarm by scoring.  Each is measured at the full-precision pose of its gso file.

  interface/buried_area.list     per candidate: swarm, glowworm, the gso file's scoring, the solvent-accessible area of the
                                 receptor alone, of the ligand alone and of the complex, and the area the interface buries
                                 (receptor + ligand - complex), in A^2 with one decimal
  interface/residues_<k>.list    with --top N, for the k-th candidate (k = 1 .. N): side (R / L), residue id and the free,
                                 bound and buried area of every residue that loses area in the complex

The library returns integer point counts weighted by the squared expanded radius; the areas are the plain functions below.
Path rules as launch.py.
"""
import math
import os
import sys

import numpy as np

try:
    from .run_dir import argument_parser, build_complex, candidates, open_run, pose_matrix, swarm_list
except ImportError:  # run as a script
    from run_dir import argument_parser, build_complex, candidates, open_run, pose_matrix, swarm_list

POINTS = 128
AREA = 4.0 * math.pi / (POINTS * 1e6)   # a weighted count (count x E^2, thousandths^2) -> A^2
BURIED_HEADER = "Swarm  Glowworm     Scoring   RecFree   LigFree   Complex    Buried\n"
RESIDUES_HEADER = "Side Residue           Free     Bound    Buried\n"


def areas(sums):
    """The four sums of one pose -> (receptor free, ligand free, complex, buried) in A^2; the differences are exact integers."""
    s = [int(v) for v in sums]
    return s[0] * AREA, s[2] * AREA, (s[1] + s[3]) * AREA, (s[0] - s[1] + s[2] - s[3]) * AREA


def buried_area_text(entries, sums):
    return BURIED_HEADER + "".join("%5d %9d %11.5f %9.1f %9.1f %9.1f %9.1f\n" % ((e[0], e[1], e[3]["scoring"]) + areas(sums[i]))
                                   for i, e in enumerate(entries))


def residue_weights(counts, radii, probe, residue_of_atom, n_residues):
    """Per-atom point counts of one side and one pose -> the weighted count sum count x E^2 of every residue (int64)."""
    p = int(round(1000.0 * probe))
    radii = np.asarray(radii, dtype=np.int64)
    E2 = np.where(radii > 0, (radii + p) ** 2, 0)
    out = np.zeros(n_residues, dtype=np.int64)
    np.add.at(out, np.asarray(residue_of_atom, dtype=np.int64), np.asarray(counts, dtype=np.int64) * E2)
    return out


def residues_text(sides):
    """sides: (("R", residue ids, free weights, bound weights), ("L", ...)).  Only residues that lose area."""
    lines = [RESIDUES_HEADER]
    for tag, ids, free, bound in sides:
        for r in np.flatnonzero(np.asarray(free) > np.asarray(bound)):
            f, b = int(free[r]), int(bound[r])
            lines.append("%s    %-12s %9.1f %9.1f %9.1f\n" % (tag, ids[r], f * AREA, b * AREA, (f - b) * AREA))
    return "".join(lines)


def parse_list(text):
    """A list written above -> (header columns, rows of strings)."""
    lines = text.splitlines()
    return lines[0].split(), [line.split() for line in lines[1:] if line.strip()]


def main(argv=None):
    ap = argument_parser()
    ap.add_argument("--probe", type=float, default=1.4, help="probe radius (A), 0 .. 2.0")
    ap.add_argument("--top", type=int, default=None, help="interface/residues_<k>.list of the first N candidates")
    args = ap.parse_args(argv)

    pkg, setup, sim = open_run(args.setup)
    cx = build_complex(pkg, setup, sim)
    entries = candidates(swarm_list(args.swarms, setup), args.step, args.all)
    poses = pose_matrix(entries, args.step, cx.pose_len)
    top = min(len(entries), max(0, args.top or 0))
    out = cx.sasa(poses, args.probe, atoms=top > 0)      # the one GPU call
    ms = cx.last_kernel_ms()

    os.makedirs("interface", exist_ok=True)
    with open(os.path.join("interface", "buried_area.list"), "w") as f:
        f.write(buried_area_text(entries, out["sums"]))
    if top:
        n_rec = cx.num_atoms(0)
        cut = {0: slice(0, n_rec), 1: slice(n_rec, None)}
        info = [(tag, cx.residues(side), cx.sasa_radii(side), cx.residue_of_atom(side)) for side, tag in enumerate("RL")]
        for k in range(top):
            sides = []
            for side, (tag, ids, radii, of) in enumerate(info):
                free, bound = (residue_weights(out[key][k, cut[side]], radii, args.probe, of, len(ids)) for key in ("free", "bound"))
                sides.append((tag, ids, free, bound))
            with open(os.path.join("interface", "residues_%d.list" % (k + 1)), "w") as f:
                f.write(residues_text(sides))
    buried = [areas(s)[3] for s in out["sums"]]
    print("%d models measured (%.3f ms of kernels)%s" % (len(entries), ms, ": %.1f ... %.1f A^2 buried" % (min(buried), max(buried)) if buried else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
