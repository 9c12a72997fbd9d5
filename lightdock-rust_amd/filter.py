"""Filter of the ranked models of a run by restraints and by membrane beads, the step that follows lgd_rank.py / lgd_top.py in
LightDock's workflow (lgd_filter_restraints.py, lgd_filter_membrane.py), with the interface contacts of ALL candidates in ONE
ld_complex_contacts call on the GPU.

    cd run_dir && python lightdock-rust_amd/filter.py <setup.json> <step> [--swarms 0-9] [--all] [--restraints FILE]
                                                       [--cutoff 5.0] [--fnat 0.4] [--max-beads N] [--write-pdb]

Candidates: the entries of rank_by_scoring.list as run_dir.ranking() forms them from swarm_<i>/cluster.repr and
gso_<step>.out (the full-precision pose of the gso file); with --all every glowworm of every selected swarm, by scoring,
highest first, ties in (swarm, glowworm) order.  Per candidate: `rec` / `lig` = the fraction of the receptor's / ligand's
restraint residues (active + passive; blocked ones are ignored) in contact with the other molecule, -1 for a side without
restraints (which is satisfied); `beads` = receptor residues named MMB (membrane beads) in contact with the ligand.  Kept:
rec >= fnat and lig >= fnat and beads <= N.  Writes filtered/rank_filtered.list and, with --write-pdb,
filtered/swarm_<s>_<g>.pdb.  The contact rule is this project's (include/lightdock_hip.h, "Interface contacts"), modelled on
LightDock's tools; its files are not claimed to equal theirs byte for byte.  Path rules as launch.py.
"""
import os
import sys

import numpy as np

try:
    from .run_dir import all_glowworms, argument_parser, build_complex, candidates, open_run, pose_matrix, swarm_list  # noqa: F401
except ImportError:  # run as a script
    from run_dir import all_glowworms, argument_parser, build_complex, candidates, open_run, pose_matrix, swarm_list  # noqa: F401

FILTER_HEADER = "Swarm  Glowworm     Scoring      Rec      Lig   Beads\n"
BEAD_RESIDUE = "MMB"   # the reference's membrane beads (src/dfire.rs:107)


def parse_restraints_list(text):
    """LightDock's restraints list, lines of `R|L <residue id> [A|P|B]` -> {"rec": [ids], "lig": [ids]} in file order.
    No flag means active; B (blocked) residues are left out; blank lines are skipped."""
    out = {"rec": [], "lig": []}
    for n, line in enumerate(text.splitlines(), 1):
        parts = line.split()
        if not parts:
            continue
        if len(parts) not in (2, 3) or parts[0] not in ("R", "L") or (len(parts) == 3 and parts[2] not in ("A", "P", "B")):
            raise ValueError("restraints list, line %d: expected 'R|L <residue id> [A|P|B]', got %r" % (n, line))
        if len(parts) == 3 and parts[2] == "B":
            continue
        out["rec" if parts[0] == "R" else "lig"].append(parts[1])
    return out


def setup_restraints(setup):
    """setup.json's restraints, active then passive -> {"rec": [ids], "lig": [ids]}."""
    out = {}
    for side, key in (("rec", "receptor_restraints"), ("lig", "ligand_restraints")):
        r = setup.get(key) or {}
        out[side] = list(r.get("active") or []) + list(r.get("passive") or [])
    return out


def restraint_columns(ids, residues, what):
    """For each restraint id, the residue indices that carry it.  An id that names no residue is an error."""
    where = {}
    for i, r in enumerate(residues):
        where.setdefault(r, []).append(i)
    missing = [r for r in ids if r not in where]
    if missing:
        raise ValueError("%s restraint(s) %s name no residue of the PDB file" % (what, ", ".join(missing)))
    return [where[r] for r in ids]


def fractions(contact, columns):
    """contact: bool (n, residues); columns: restraint_columns() -> per pose the fraction of restraint residues in contact,
    -1.0 everywhere for a side without restraints."""
    contact = np.asarray(contact, dtype=bool)
    if not columns:
        return np.full(contact.shape[0], -1.0)
    hits = np.stack([contact[:, c].any(axis=1) for c in columns], axis=1)
    return hits.sum(axis=1) / float(len(columns))


def bead_counts(rec_contact, rec_residues):
    """Receptor residues named MMB in contact with the ligand, per pose."""
    beads = np.array([r.split(".")[1] == BEAD_RESIDUE for r in rec_residues], dtype=bool)
    return np.asarray(rec_contact, dtype=bool)[:, beads].sum(axis=1).astype(np.int64)


def keep_mask(rec, lig, beads, fnat, max_beads=None):
    """A side without restraints (-1) is satisfied."""
    keep = ((rec < 0) | (rec >= fnat)) & ((lig < 0) | (lig >= fnat))
    return keep if max_beads is None else keep & (beads <= max_beads)


def rank_filtered_text(entries, rec, lig, beads, keep):
    return FILTER_HEADER + "".join("%5d %9d %11.5f %8.3f %8.3f %7d\n" % (e[0], e[1], e[3]["scoring"], rec[i], lig[i], beads[i])
                                   for i, e in enumerate(entries) if keep[i])


def main(argv=None):
    ap = argument_parser()
    ap.add_argument("--restraints", default=None, help="a LightDock restraints list instead of setup.json's restraints")
    ap.add_argument("--cutoff", type=float, default=5.0, help="contact distance (A)")
    ap.add_argument("--fnat", type=float, default=0.4, help="least fraction of restraint residues in contact, per side")
    ap.add_argument("--max-beads", type=int, default=None, help="most membrane beads in contact with the ligand")
    ap.add_argument("--write-pdb", action="store_true", help="filtered/swarm_<s>_<g>.pdb of every kept model")
    args = ap.parse_args(argv)

    pkg, setup, sim = open_run(args.setup)
    cx = build_complex(pkg, setup, sim)

    wanted = parse_restraints_list(open(args.restraints).read()) if args.restraints else setup_restraints(setup)
    residues = {"rec": cx.residues(0), "lig": cx.residues(1)}
    columns = {"rec": restraint_columns(wanted["rec"], residues["rec"], "receptor"),
               "lig": restraint_columns(wanted["lig"], residues["lig"], "ligand")}

    entries = candidates(swarm_list(args.swarms, setup), args.step, args.all)
    poses = pose_matrix(entries, args.step, cx.pose_len)
    contact = cx.contacts(poses, args.cutoff)
    rec, lig = fractions(contact["rec"], columns["rec"]), fractions(contact["lig"], columns["lig"])
    beads = bead_counts(contact["rec"], residues["rec"])
    keep = keep_mask(rec, lig, beads, args.fnat, args.max_beads)

    os.makedirs("filtered", exist_ok=True)
    with open(os.path.join("filtered", "rank_filtered.list"), "w") as f:
        f.write(rank_filtered_text(entries, rec, lig, beads, keep))
    if args.write_pdb:
        for i in np.flatnonzero(keep):
            cx.write_pdb(poses[i], os.path.join("filtered", "swarm_%d_%d.pdb" % entries[i][:2]))
    print("%d of %d models kept" % (int(keep.sum()), len(entries)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
