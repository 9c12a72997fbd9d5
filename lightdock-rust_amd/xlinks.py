"""The chemical cross-links (XL-MS) of every model of a run, with ALL candidates in ONE ld_complex_crosslinks call on the GPU
(include/lightdock_hip.h, "Cross-links": for every link the straight distance of its two atoms and the length of the
shortest path between them that stays in the solvent, on a lattice of the integer thousandths "%8.3f" prints -- the
solvent-accessible surface distance of Xwalk and Jwalk, exact integers).

    cd run_dir && python lightdock-rust_amd/xlinks.py <setup.json> <step> --links FILE [--swarms 0-9] [--all]
                              [--straight-only] [--probe 0] [--cell 1.0] [--reach 3.0] [--max-length 35] [--top N]

The link file: one link a line, "R|L <residue id> <atom name> R|L <residue id> <atom name> <limit in A>", R the receptor
and L the ligand, residue ids as in the restraint lists ("A.LYS.45"); "#" starts a comment.  A residue or an atom that
names no record of its file, or more than one, is an error that cites the line.

Candidates as ccs.py: the entries run_dir.ranking() forms from swarm_<i>/cluster.repr and gso_<step>.out, or with --all
every glowworm of every selected swarm by scoring.  Each is measured at the full-precision pose of its gso file.  A link
is satisfied when its path is at most its limit (with --straight-only, which runs no search: its straight distance); its
violation is max(0, d - limit), and a link without a path of --max-length at most counts max(0, max_length - limit).

  xlinks/rank_xlinks.list   per candidate: swarm, glowworm, the gso file's scoring, satisfied / L, satisfied by the straight
                            distance / L, the sum of the violations (A).  Rows by satisfied descending, then violation
                            ascending, then the scoring rank.
  xlinks/links.list         with --top N, every link of the first N rows: its straight distance, its path ("-" without
                            one, or with --straight-only) and its limit
  xlinks/model_<k>.pdb      with --top N, the k-th row's model (k = 1 .. N)

The probe (default 0), the reach of a side chain (default 3 A) and the lattice step are parameters of the method, not
measurements; a path over the 26 neighbours of a lattice overestimates the true geodesic by a few percent.  Path rules as
launch.py.
"""
import os
import sys

import numpy as np

try:
    from .run_dir import argument_parser, build_complex, candidates, open_run, pose_matrix, swarm_list
except ImportError:  # run as a script
    from run_dir import argument_parser, build_complex, candidates, open_run, pose_matrix, swarm_list

NO_PATH = 0xFFFFFFFF
HEADER = "Swarm  Glowworm     Scoring  Satisfied   Straight   Violation\n"
LINKS_HEADER = "Model  Link                                         Straight       Path    Limit\n"


def atom_names(pdb_path):
    """The atom name (columns 13-16, trimmed) of every ATOM / HETATM record, in file order."""
    return [line[12:16].strip() for line in open(pdb_path) if line.startswith(("ATOM  ", "HETATM"))]


def atom_table(residue_ids, residue_of_atom, names):
    """[(residue id, atom name)] of one side's atoms in file order."""
    if len(residue_of_atom) != len(names):
        raise ValueError("%d atom names for %d atoms" % (len(names), len(residue_of_atom)))
    return [(residue_ids[int(r)], name) for r, name in zip(residue_of_atom, names)]


def parse_links(text, rec_atoms, lig_atoms):
    """The link file's text, the two atom_table()s -> (links [(a, b)] of complex atom indices, limits [A], labels).
    ValueError citing the line for a line that does not parse or names no record, or more than one."""
    tables = {"R": (rec_atoms, 0), "L": (lig_atoms, len(rec_atoms))}
    links, limits, labels = [], [], []
    for number, line in enumerate(text.splitlines(), 1):
        fields = line.split("#", 1)[0].split()
        if not fields:
            continue
        if len(fields) != 7 or fields[0] not in tables or fields[3] not in tables:
            raise ValueError("line %d: expected 'R|L <residue id> <atom name> R|L <residue id> <atom name> <limit>'" % number)
        try:
            limit = float(fields[6])
        except ValueError:
            limit = float("nan")
        if not (limit >= 0.0 and limit < 1e6):
            raise ValueError("line %d: the limit '%s' is not a distance in A" % (number, fields[6]))
        pair = []
        for side, residue, name in (fields[0:3], fields[3:6]):
            table, offset = tables[side]
            if not any(r == residue for r, _ in table):
                raise ValueError("line %d: no residue %s in the %s" % (number, residue, "receptor" if side == "R" else "ligand"))
            found = [k for k, (r, a) in enumerate(table) if r == residue and a == name]
            if len(found) != 1:
                raise ValueError("line %d: %s atom %s of residue %s" % (number, "no" if not found else "more than one", name, residue))
            pair.append(offset + found[0])
        links.append(tuple(pair))
        limits.append(limit)
        labels.append("%s:%s:%s-%s:%s:%s" % tuple(fields[:6]))
    if not links:
        raise ValueError("the link file names no link")
    return links, limits, labels


def distances(straight2, path=None):
    """straight2 (n, L) uint64, path (n, L) uint32 or None -> (straight, path) in A, float64 (n, L); inf without a path."""
    straight = np.sqrt(np.asarray(straight2, dtype=np.float64)) / 1000.0
    if path is None:
        return straight, None
    path = np.asarray(path, dtype=np.uint32)
    return straight, np.where(path == NO_PATH, np.inf, path.astype(np.float64) / 1000.0)


def judge(straight, path, limits, max_length):
    """-> (satisfied (n,), satisfied by the straight distance (n,), sum of violations (n,)); the judged distance is the path,
    or the straight distance when path is None."""
    limits = np.asarray(limits, dtype=np.float64)[None, :]
    by_straight = (straight <= limits).sum(axis=1)
    d = straight if path is None else np.where(np.isinf(path), max_length, path)
    found = np.ones_like(straight, dtype=bool) if path is None else ~np.isinf(path)
    return ((d <= limits) & found).sum(axis=1), by_straight, np.maximum(0.0, d - limits).sum(axis=1)


def rank_rows(satisfied, violation):
    """Indices by satisfied descending, then violation ascending, then the entries' own order (the scoring rank)."""
    return sorted(range(len(satisfied)), key=lambda i: (-int(satisfied[i]), float(violation[i]), i))


def rank_text(entries, order, satisfied, by_straight, violation, n_links):
    rows = ["%5d %9d %11.5f %6d/%-4d %6d/%-4d %10.3f\n" % (entries[i][0], entries[i][1], entries[i][3]["scoring"], satisfied[i], n_links,
                                                         by_straight[i], n_links, violation[i]) for i in order]
    return HEADER + "".join(rows)


def links_text(order, labels, limits, straight, path):
    rows = []
    for k, i in enumerate(order, 1):
        for l, label in enumerate(labels):
            shown = "-" if path is None or np.isinf(path[i][l]) else "%.3f" % path[i][l]
            rows.append("%5d  %-40s %12.3f %10s %8.3f\n" % (k, label, straight[i][l], shown, limits[l]))
    return LINKS_HEADER + "".join(rows)


def main(argv=None):
    ap = argument_parser()
    ap.add_argument("--links", required=True, help="the link file: R|L <residue id> <atom name> R|L <residue id> <atom name> <limit in A>")
    ap.add_argument("--straight-only", action="store_true", help="judge the straight distance; no path search runs")
    ap.add_argument("--probe", type=float, default=0.0, help="probe radius (A), 0 .. 2.0: a parameter of the method")
    ap.add_argument("--cell", type=float, default=1.0, help="lattice step (A), 0.5 .. 2.0")
    ap.add_argument("--reach", type=float, default=3.0, help="how far an anchor's doors may lie (A), up to 6.0: the side chain")
    ap.add_argument("--max-length", type=float, default=35.0, help="the longest path looked for (A), up to 60 and 80 cells")
    ap.add_argument("--top", type=int, default=0, help="xlinks/links.list and xlinks/model_<k>.pdb of the first N rows")
    args = ap.parse_args(argv)
    links_path = os.path.abspath(args.links)

    pkg, setup, sim = open_run(args.setup)
    cx = build_complex(pkg, setup, sim)
    tables = [atom_table(cx.residues(side), cx.residue_of_atom(side), atom_names(os.path.join(sim, "lightdock_" + setup[key])))
              for side, key in ((0, "receptor_pdb"), (1, "ligand_pdb"))]
    try:
        links, limits, labels = parse_links(open(links_path).read(), tables[0], tables[1])
    except ValueError as e:
        raise SystemExit("%s: %s" % (args.links, e))
    entries = candidates(swarm_list(args.swarms, setup), args.step, args.all)
    poses = pose_matrix(entries, args.step, cx.pose_len)
    got = cx.crosslinks(poses, links, args.probe, args.cell, args.reach, args.max_length, paths=not args.straight_only)   # the one GPU call
    ms = cx.last_kernel_ms()
    straight, path = distances(got["straight2"], got.get("path"))
    satisfied, by_straight, violation = judge(straight, path, limits, args.max_length)
    order = rank_rows(satisfied, violation)

    os.makedirs("xlinks", exist_ok=True)
    with open(os.path.join("xlinks", "rank_xlinks.list"), "w") as f:
        f.write(rank_text(entries, order, satisfied, by_straight, violation, len(links)))
    top = order[:max(0, args.top)]
    if top:
        with open(os.path.join("xlinks", "links.list"), "w") as f:
            f.write(links_text(top, labels, limits, straight, path))
    for k, i in enumerate(top, 1):
        cx.write_pdb(poses[i], os.path.join("xlinks", "model_%d.pdb" % k))
    print("%d models, %d links measured (%.3f ms of device work, %s, cell %.3f A, probe %.3f A, reach %.3f A)%s"
          % (len(entries), len(links), ms, "straight distances only" if args.straight_only else "paths up to %.1f A" % args.max_length,
             args.cell, args.probe, args.reach, ": %d ... %d satisfied" % (satisfied.min(), satisfied.max()) if len(entries) else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
