"""Prepares a run from its two PDB files: what lightdock3_setup.py does before `launch.py` / `lightdock-hip` can start.

    python lightdock-rust_amd/prepare.py REC.pdb LIG.pdb [-s N] [--max-swarms 400] [-g 200] [--seed 324324]
           [--anm] [--anm-rec 10] [--anm-lig 10] [--anm-rec-rmsd 0.5] [--anm-lig-rmsd 0.5] [-r RESTRAINTS] [--membrane]
           [--keep-h] [--keep-oxt] [--keep-waters] [--spacing 2.0] [--swarm-radius 10] [--swarms-per-restraint 20]
           [--out DIR] [--force]

Writes into DIR (default: the CWD) the cleaned, centred lightdock_<rec>, lightdock_<lig>, setup.json, init/swarm_centers.pdb
and init/initial_positions_<i>.dat; with --anm then the four mode files of anm.py.  The swarm centres are this project's
own integer rule (include/lightdock_hip.h, "Preparing a run"), modelled on LightDock's and not claimed to
equal it: a shell of lattice nodes around the receptor at the distance D the ligand's size gives, thinned by farthest-point
sampling on the GPU, then filtered by the receptor's restraints.  -s N asks for exactly N centres before that filter;
without it centres are added until every candidate lies within the swarm radius of one, --max-swarms at most.  RESTRAINTS
is a list in filter.py's format.  Refuses to overwrite anything without --force, before anything is computed.
"""
import argparse
import glob
import json
import math
import os
import shutil
import sys

import numpy as np

BEAD_RESIDUE = "MMB"
BEAD_RADIUS = 2000        # thousandths: a bead's extent is 2000 + D
SETUP_VERSION = "0.9.4"   # the LightDock setup.json this file follows
SIDES = ("rec", "lig")


def argument_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("receptor")
    ap.add_argument("ligand")
    ap.add_argument("-s", "--swarms", type=int, default=None, help="exactly N centres before the restraint filter")
    ap.add_argument("--max-swarms", type=int, default=400, help="most centres of the cover rule")
    ap.add_argument("-g", "--glowworms", type=int, default=200)
    ap.add_argument("--seed", type=int, default=324324, help="starting_points_seed")
    ap.add_argument("--anm", action="store_true", help="use_anm: poses carry mode extents and anm.py writes the mode files")
    ap.add_argument("--anm-rec", type=int, default=10)
    ap.add_argument("--anm-lig", type=int, default=10)
    ap.add_argument("--anm-rec-rmsd", type=float, default=0.5)
    ap.add_argument("--anm-lig-rmsd", type=float, default=0.5)
    ap.add_argument("-r", "--restraints", default=None, help="a LightDock restraints list: R|L <residue id> [A|P|B]")
    ap.add_argument("--membrane", action="store_true", help="recorded in setup.json; MMB beads keep centres out either way")
    ap.add_argument("--keep-h", action="store_true")
    ap.add_argument("--keep-oxt", action="store_true")
    ap.add_argument("--keep-waters", action="store_true")
    ap.add_argument("--spacing", type=float, default=2.0, help="lattice spacing of the shell (A)")
    ap.add_argument("--swarm-radius", type=float, default=10.0, help="radius of a swarm's start translations and of the cover rule (A)")
    ap.add_argument("--swarms-per-restraint", type=int, default=20)
    ap.add_argument("--out", default=".", help="the run's directory")
    ap.add_argument("--force", action="store_true", help="overwrite files that exist")
    return ap


def parse_restraints(text):
    """LightDock's restraints list -> {"rec": {"active", "passive", "blocked"}, "lig": ...}, ids in file order."""
    out = {side: {"active": [], "passive": [], "blocked": []} for side in SIDES}
    kinds = {"A": "active", "P": "passive", "B": "blocked"}
    for n, line in enumerate(text.splitlines(), 1):
        parts = line.split()
        if not parts:
            continue
        if len(parts) not in (2, 3) or parts[0] not in ("R", "L") or (len(parts) == 3 and parts[2] not in kinds):
            raise ValueError("restraints list, line %d: expected 'R|L <residue id> [A|P|B]', got %r" % (n, line))
        out["rec" if parts[0] == "R" else "lig"][kinds[parts[2]] if len(parts) == 3 else "active"].append(parts[1])
    return out


def records(path):
    return [line.rstrip("\r\n") for line in open(path) if line.startswith(("ATOM  ", "HETATM"))]


def thousandths(recs):
    """(n, 3) int64: the coordinates as "%8.3f" printed them."""
    return np.array([[int(round(float(r[30 + 8 * c:38 + 8 * c]) * 1000.0)) for c in range(3)] for r in recs], dtype=np.int64).reshape(-1, 3)


def residue_id(record):
    """"<chain>.<resname>.<serial><icode>", as the library's residue ids."""
    return "%s.%s.%d%s" % (record[21:22].strip(), record[17:20].strip(), int(record[22:26]), record[26:27].strip())


def restraint_atoms(recs, ids, what):
    """For each id the record index of its residue's CA, else P, else first atom.  An id that names no residue is an error."""
    first, ca, p = {}, {}, {}
    for a, r in enumerate(recs):
        rid, name = residue_id(r), r[12:16].strip()
        first.setdefault(rid, a)
        if name == "CA":
            ca.setdefault(rid, a)
        if name == "P":
            p.setdefault(rid, a)
    missing = [i for i in ids if i not in first]
    if missing:
        raise ValueError("%s restraint(s) %s name no residue of the PDB file" % (what, ", ".join(missing)))
    return [ca.get(i, p.get(i, first[i])) for i in ids]


def radii(recs):
    """The surface rule's radius of every record, thousandths; 0: takes no part (hydrogen, bead)."""
    table = {"C": 1700, "N": 1550, "O": 1520, "F": 1470, "P": 1800, "S": 1800, "CL": 1750, "SE": 1900, "BR": 1850, "I": 1980}
    out = []
    for r in recs:
        e = r[76:78].strip().upper() if len(r) >= 78 else ""
        if not e:
            e = next((ch for ch in r[12:16] if ch.isalpha()), "").upper()
        out.append(0 if e in ("H", "D") or r[17:20].strip() == BEAD_RESIDUE else table.get(e, 1800))
    return np.array(out, dtype=np.int64)


def shell_atoms(recs, xyz, D):
    """(atoms (m, 4) int32 x y z E, bead flags): atoms with a radius get R + D, MMB beads 2000 + D and the flag."""
    R = radii(recs)
    bead = np.array([r[17:20].strip() == BEAD_RESIDUE for r in recs], dtype=bool)
    R = np.where(bead, BEAD_RADIUS, R)
    part = R > 0
    atoms = np.concatenate([xyz[part], (R[part] + D)[:, None]], axis=1)
    return atoms.astype(np.int32), bead[part].astype(np.uint8)


def restraint_filter(centres, points, per_restraint):
    """Indices, ascending, of the centres among the per_restraint nearest to some restraint point, ties by centre index."""
    keep = set()
    for r in points:
        d2 = ((centres - r) ** 2).sum(axis=1)
        keep.update(np.lexsort((np.arange(len(centres)), d2))[:per_restraint].tolist())
    return sorted(keep)


def setup_dict(args, rec_name, lig_name, restraints, swarms):
    """Every key of a LightDock setup.json, the non-optional fields of the reference's SetupFile among them."""
    return {
        "anm_lig": args.anm_lig, "anm_lig_rmsd": args.anm_lig_rmsd, "anm_rec": args.anm_rec, "anm_rec_rmsd": args.anm_rec_rmsd,
        "anm_seed": args.seed, "dense_sampling": False, "fixed_distance": 0.0, "flip": False, "glowworms": args.glowworms,
        "ligand_pdb": lig_name, "ligand_restraints": restraints["lig"], "membrane": bool(args.membrane), "noh": not args.keep_h,
        "now": not args.keep_waters, "noxt": not args.keep_oxt, "receptor_pdb": rec_name, "receptor_restraints": restraints["rec"],
        "restraints": os.path.basename(args.restraints) if args.restraints else None, "setup_version": SETUP_VERSION,
        "starting_points_seed": args.seed, "surface_density": 50.0, "swarm_radius": args.swarm_radius, "swarms": swarms,
        "swarms_per_restraint": args.swarms_per_restraint, "transmembrane": False, "use_anm": bool(args.anm), "verbose_parser": False,
        "write_starting_positions": False,
    }


def positions_text(rows):
    """Space separated "%.9f", no trailing blank: the reference splits a line on single spaces."""
    return "".join(" ".join("%.9f" % v for v in row) + "\n" for row in rows)


def centres_pdb_text(centres):
    """init/swarm_centers.pdb: one pseudo-atom a centre, coordinates in A."""
    return "".join("HETATM%5d   H  SWR Z%4d    %8.3f%8.3f%8.3f\n" % ((i + 1) % 100000, (i + 1) % 10000, c[0], c[1], c[2])
                   for i, c in enumerate(centres))


def planned_outputs(out, rec_name, lig_name, anm):
    files = [os.path.join(out, "lightdock_" + rec_name), os.path.join(out, "lightdock_" + lig_name), os.path.join(out, "setup.json"),
             os.path.join(out, "init", "swarm_centers.pdb")]
    files += sorted(glob.glob(os.path.join(out, "init", "initial_positions_*.dat")))
    if anm:
        files += [os.path.join(out, f) for f in ("lightdock_rec.nm.npy", "rec_nm.npy", "lightdock_lig.nm.npy", "lig_nm.npy")]
    return files


def write_run(out, setup, centres, rows):
    """setup.json and init/ of a run: centres (n, 3) in A, rows[i] the pose rows of swarm i.  Stale initial_positions files go."""
    os.makedirs(os.path.join(out, "init"), exist_ok=True)
    for stale in glob.glob(os.path.join(out, "init", "initial_positions_*.dat")):
        os.remove(stale)
    with open(os.path.join(out, "setup.json"), "w") as f:
        json.dump(setup, f, indent=4, sort_keys=True)
        f.write("\n")
    with open(os.path.join(out, "init", "swarm_centers.pdb"), "w") as f:
        f.write(centres_pdb_text(centres))
    for i, block in enumerate(rows):
        with open(os.path.join(out, "init", "initial_positions_%d.dat" % i), "w") as f:
            f.write(positions_text(block))


def swarm_centres(pkg, rec, lig, spacing, radius, n_swarms, max_swarms):
    """Rules 1-3 on the records of the two cleaned files.  Returns a dict: D, nodes, candidates (n, 3), index, gap2, ms."""
    lig_xyz = thousandths(lig)[radii(lig) > 0]
    if len(lig_xyz) == 0:
        raise ValueError("no ligand atom has a radius")
    d2 = pkg.swarm_diameter2(lig_xyz.astype(np.int32))
    ms = pkg.setup_last_kernel_ms()
    D = math.isqrt(d2) // 4
    atoms, bead = shell_atoms(rec, thousandths(rec), D)
    if len(atoms) == 0 or bead.all():
        raise ValueError("no receptor atom has a radius")
    candidates, nodes = pkg.swarm_shell(atoms, bead, spacing, lattice_nodes=True)
    ms += pkg.setup_last_kernel_ms()
    if len(candidates) == 0:
        raise ValueError("the shell has no candidate node: lower --spacing")
    if n_swarms is not None:
        index, gap2 = pkg.swarm_centres(candidates, n_swarms, 0)
    else:
        index, gap2 = pkg.swarm_centres(candidates, max_swarms, radius)
    ms += pkg.setup_last_kernel_ms()
    return {"D": D, "nodes": nodes, "candidates": candidates, "index": index, "gap2": gap2, "ms": ms}


def main(argv=None):
    args = argument_parser().parse_args(argv)
    out = args.out
    rec_name, lig_name = os.path.basename(args.receptor), os.path.basename(args.ligand)
    spacing, radius = int(round(args.spacing * 1000.0)), int(round(args.swarm_radius * 1000.0))
    if args.glowworms < 1 or args.max_swarms < 1 or (args.swarms is not None and args.swarms < 1) or args.swarms_per_restraint < 1:
        print("prepare.py: swarms, glowworms and swarms per restraint must be positive", file=sys.stderr)
        return 1
    existing = [p for p in planned_outputs(out, rec_name, lig_name, args.anm) if os.path.exists(p)]
    if existing and not args.force:
        print("prepare.py: %s exist%s; --force overwrites" % (", ".join(existing), "s" if len(existing) == 1 else ""), file=sys.stderr)
        return 1
    restraints = parse_restraints(open(args.restraints).read()) if args.restraints else parse_restraints("")

    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    import __graft_entry__ as ge
    pkg = ge.package()
    pkg.init(-1)

    os.makedirs(out, exist_ok=True)
    paths = {"rec": os.path.join(out, "lightdock_" + rec_name), "lig": os.path.join(out, "lightdock_" + lig_name)}
    for side, src in (("rec", args.receptor), ("lig", args.ligand)):
        atoms, centre = pkg.prepare_pdb(src, paths[side], args.keep_h, args.keep_oxt, args.keep_waters)
        print("%s: %d atoms kept, centre (%.3f, %.3f, %.3f) -> %s" % (os.path.basename(src), atoms, centre[0], centre[1], centre[2], paths[side]))
    if args.restraints and os.path.abspath(args.restraints) != os.path.abspath(os.path.join(out, os.path.basename(args.restraints))):
        shutil.copy(args.restraints, os.path.join(out, os.path.basename(args.restraints)))
    recs = {side: records(paths[side]) for side in SIDES}
    wanted = {side: restraints[side]["active"] + restraints[side]["passive"] for side in SIDES}
    what = {"rec": "receptor", "lig": "ligand"}
    for side in SIDES:   # a blocked id must name a residue too
        restraint_atoms(recs[side], restraints[side]["blocked"], what[side])
    points = {side: thousandths(recs[side])[restraint_atoms(recs[side], wanted[side], what[side])].reshape(-1, 3) for side in SIDES}

    found = swarm_centres(pkg, recs["rec"], recs["lig"], spacing, radius, args.swarms, args.max_swarms)
    centres = found["candidates"][found["index"]].astype(np.int64)
    picked = len(centres)
    if len(points["rec"]):
        centres = centres[restraint_filter(centres, points["rec"], args.swarms_per_restraint)]
    cover = float(np.sqrt(float(found["gap2"][-1]))) / 1000.0 if picked > 1 else 0.0
    print("D %d, %d nodes, %d candidates, %d centres (%d after the restraint filter), cover radius %.3f A, %.2f ms on the device" %
          (found["D"], found["nodes"], len(found["candidates"]), picked, len(centres), cover, found["ms"]))

    centres_a = centres / 1000.0
    anm = (args.anm_rec, args.anm_lig) if args.anm else (0, 0)
    rows = [pkg.initial_poses(args.seed, args.glowworms, s, centres_a[s], radius=args.swarm_radius, rec_points=points["rec"] / 1000.0,
                              lig_points=points["lig"] / 1000.0, anm_rec=anm[0], anm_lig=anm[1])[0] for s in range(len(centres))]
    setup = setup_dict(args, rec_name, lig_name, restraints, len(centres))
    write_run(out, setup, centres_a, rows)
    print("%d swarms of %d glowworms -> %s, %s" % (len(centres), args.glowworms, os.path.join(out, "setup.json"), os.path.join(out, "init")))

    if args.anm:
        try:
            from . import anm as anm_tool
        except ImportError:  # run as a script
            import anm as anm_tool
        back = os.getcwd()
        os.chdir(out)
        try:
            return anm_tool.main(["setup.json", "--rmsd"] + (["--force"] if args.force else []))
        finally:
            os.chdir(back)
    return 0


if __name__ == "__main__":
    sys.exit(main())
