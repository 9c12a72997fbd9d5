"""Why a model scored as it did: the terms of its energy and the residues that carry it, for the ranked models of a run,
with ALL candidates in ONE ld_scorer_decompose call on the GPU (include/lightdock_hip.h, "Energy decomposition").

    cd run_dir && python lightdock-rust_amd/decompose.py <setup.json> <step> <dfire|dna|pydock> [--swarms 0-9] [--all] [--top N]

The scorer is built as launch.py builds it (setup.json's restraints and ANM, DCparams for DFIRE).  Candidates as filter.py:
the entries run_dir.ranking() forms from swarm_<i>/cluster.repr and gso_<step>.out, or with --all every glowworm of every
selected swarm by scoring; --top N keeps the first N.  Each is decomposed at the full-precision pose of its gso file.

  decomposition/terms.list      per candidate: swarm, glowworm, the gso file's scoring, energy, score, the pair terms (DFIRE:
                                the table sum; DNA / PYDOCK: electrostatics and van der Waals, raw), the fractions of receptor
                                and ligand restraints satisfied, the fraction of membrane beads at the interface, the
                                penalty subtracted for them, pairs inside the cutoff
  decomposition/residues.list   per candidate, side (R / L) and residue with a pair inside the cutoff: its energy in SCORE
                                units (DFIRE: -0.0157 x sum; DNA / PYDOCK: -332/4 x electrostatics, -van der Waals and their
                                sum), pairs, interface atoms.  A side's residues add up to the candidate's score (DFIRE: less
                                the constant 4.7).

Residues are those of the scoring model's atom walk (ld_model_residue_of_atom).  The library returns raw sums; the scaling
to score units is the plain functions below.  Path rules as launch.py.
"""
import os
import sys

import numpy as np

try:
    from .run_dir import argument_parser, build_scorer, candidates, open_run, pose_matrix, swarm_list
except ImportError:  # run as a script
    from run_dir import argument_parser, build_scorer, candidates, open_run, pose_matrix, swarm_list

MEMBRANE_PENALTY_SCORE = 999.0   # src/constants.rs
# energies are printed with 17 significant digits: the lists hold the doubles the library returned
TERMS_HEADER = {True: "Swarm Glowworm Scoring Energy Score Pair Rec Lig Beads Penalty Pairs\n",
                False: "Swarm Glowworm Scoring Energy Score Elec VdW Rec Lig Beads Penalty Pairs\n"}
RESIDUES_HEADER = {True: "Swarm Glowworm Side Residue Energy Pairs Interface\n",
                   False: "Swarm Glowworm Side Residue Elec VdW Energy Pairs Interface\n"}


def score_units(sums, dfire):
    """Raw group sums (..., 2) -> score units (..., columns): DFIRE one column, -0.0157 x sum (src/dfire.rs:347 without its
    constant); DNA / PYDOCK three: -332/4 x electrostatics, -van der Waals, their sum (src/dna.rs:513-514)."""
    sums = np.asarray(sums, dtype=np.float64)
    if dfire:
        return sums[..., :1] * 0.0157 * -1.0
    elec = sums[..., 0] * 332.0 / 4.0 * -1.0
    vdw = sums[..., 1] * -1.0
    return np.stack([elec, vdw, elec + vdw], axis=-1)


def penalty(beads_fraction):
    """src/dfire.rs:355-359."""
    beads_fraction = np.asarray(beads_fraction, dtype=np.float64)
    return np.where(beads_fraction > 0.0, MEMBRANE_PENALTY_SCORE * beads_fraction, 0.0)


def terms_text(entries, terms, dfire):
    lines = [TERMS_HEADER[dfire]]
    pen = penalty(terms["membrane"])
    for i, e in enumerate(entries):
        t = terms[i]
        pair = "%24.17g" % t["pair"][0] if dfire else "%24.17g %24.17g" % (t["pair"][0], t["pair"][1])
        lines.append("%5d %5d %12.5f %24.17g %24.17g %s %8.6f %8.6f %8.6f %24.17g %9d\n"
                     % (e[0], e[1], e[3]["scoring"], t["energy"], t["score"], pair, t["rec_restraints"], t["lig_restraints"],
                        t["membrane"], pen[i], t["pairs"]))
    return "".join(lines)


def residues_text(entries, sides, dfire):
    """sides: (("R", residue ids, decompose()'s dict of that side), ("L", ...)).  Only residues with a pair inside the cutoff."""
    lines = [RESIDUES_HEADER[dfire]]
    units = [score_units(side[2]["sums"], dfire) for side in sides]
    for i, e in enumerate(entries):
        for (tag, ids, res), u in zip(sides, units):
            for r in np.flatnonzero(np.asarray(res["pairs"][i]) > 0):
                lines.append("%5d %5d %s %-12s %s %8d %6d\n" % (e[0], e[1], tag, ids[r], " ".join("%24.17g" % v for v in u[i, r]),
                                                                 res["pairs"][i, r], res["interface"][i, r]))
    return "".join(lines)


def parse_list(text):
    """A list written above -> (header columns, rows of strings)."""
    lines = text.splitlines()
    return lines[0].split(), [line.split() for line in lines[1:] if line.strip()]


def main(argv=None):
    ap = argument_parser()
    ap.add_argument("method")
    ap.add_argument("--top", type=int, default=None, help="only the first N candidates")
    args = ap.parse_args(argv)

    pkg, setup, sim = open_run(args.setup)
    method = args.method.lower()
    dfire = method == "dfire"
    scorer = build_scorer(pkg, setup, sim, method)
    models = [pkg.model_from_pdb(method, os.path.join(sim, "lightdock_" + setup[key])) for key in ("receptor_pdb", "ligand_pdb")]

    entries = candidates(swarm_list(args.swarms, setup), args.step, args.all)
    if args.top is not None:
        entries = entries[:max(0, args.top)]
    poses = pose_matrix(entries, args.step, scorer.pose_len)
    out = scorer.decompose(poses, rec_groups=models[0]["residue_of_atom"], lig_groups=models[1]["residue_of_atom"])

    os.makedirs("decomposition", exist_ok=True)
    with open(os.path.join("decomposition", "terms.list"), "w") as f:
        f.write(terms_text(entries, out["terms"], dfire))
    with open(os.path.join("decomposition", "residues.list"), "w") as f:
        f.write(residues_text(entries, (("R", models[0]["residues"], out["rec"]), ("L", models[1]["residues"], out["lig"])), dfire))
    print("%d models decomposed (%.3f ms of kernels)" % (len(entries), scorer.decompose_info()["last_kernel_ms"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
