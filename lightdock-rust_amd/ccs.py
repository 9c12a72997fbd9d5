"""The ion-mobility collision cross-section (CCS) of every model of a run, with ALL candidates in ONE ld_complex_ccs call on
the GPU (include/lightdock_hip.h, "Collision cross-section": the projection approximation on the integer thousandths
"%8.3f" prints -- the covered points of a fixed lattice in 64 fixed views, exact counts).

    cd run_dir && python lightdock-rust_amd/ccs.py <setup.json> <step> [--swarms 0-9] [--all] [--probe 1.0] [--cell 0.5]
                                                   [--experimental X [--sigma S] [--scale K]] [--top N]

Candidates as saxs.py: the entries run_dir.ranking() forms from swarm_<i>/cluster.repr and gso_<step>.out, or with --all
every glowworm of every selected swarm by scoring.  Each is measured at the full-precision pose of its gso file.

  ccs/rank_ccs.list     two header lines "# receptor alone ..." and "# ligand alone ..." (the ligand at the first ranked pose:
                        its lattice points move with the pose), then per candidate: swarm, glowworm, the gso file's scoring,
                        CCS_PA and the smallest and largest view area (A^2); with --experimental X (A^2) also K CCS_PA - X and
                        the same over --sigma S (default 1).  K (--scale, default 1.0) is the calibration of the projection
                        approximation to the experiment, the user's to choose: the two header lines are there to find it
                        from the monomers' measured values.  Rows by |K CCS_PA - X| ascending, ties in the order of the
                        scoring rank; without --experimental the scoring rank is kept.
  ccs/model_<k>.pdb     with --top N, the k-th row's model (k = 1 .. N)

The probe (default 1.0 A) is a parameter of the method, not a measurement.  Path rules as launch.py.
"""
import os
import sys

import numpy as np

try:
    from .run_dir import argument_parser, build_complex, candidates, open_run, pose_matrix, swarm_list
except ImportError:  # run as a script
    from run_dir import argument_parser, build_complex, candidates, open_run, pose_matrix, swarm_list

VIEWS = 64
HEADER = "Swarm  Glowworm     Scoring      CCS_PA   MinView   MaxView\n"
HEADER_EXP = "Swarm  Glowworm     Scoring      CCS_PA   MinView   MaxView      Delta   Delta/S\n"


def areas(counts, h):
    """counts (n, 64) of covered lattice points, the step h in thousandths -> (CCS_PA, smallest view, largest view), A^2 each (n,)."""
    counts = np.asarray(counts, dtype=np.uint64).reshape(-1, VIEWS)
    unit = float(h * h) / 1e6
    return counts.sum(axis=1).astype(np.float64) * unit / VIEWS, counts.min(axis=1).astype(np.float64) * unit, counts.max(axis=1).astype(np.float64) * unit


def deltas(ccs, experimental, scale=1.0):
    """K CCS_PA - X."""
    return scale * np.asarray(ccs, dtype=np.float64) - experimental


def rank_rows(n, delta=None):
    """Indices of the n entries by |delta| ascending, ties in the entries' own order (the scoring rank); without delta that order."""
    return list(range(n)) if delta is None else sorted(range(n), key=lambda i: abs(delta[i]))


def monomer_text(name, ccs, smallest, largest):
    return "# %-8s alone: CCS_PA %10.2f A^2, views %10.2f .. %10.2f\n" % (name, ccs, smallest, largest)


def rank_text(entries, order, ccs, smallest, largest, delta=None, sigma=1.0):
    rows = []
    for i in order:
        row = "%5d %9d %11.5f %11.2f %9.2f %9.2f" % (entries[i][0], entries[i][1], entries[i][3]["scoring"], ccs[i], smallest[i], largest[i])
        if delta is not None:
            row += " %10.2f %9.3f" % (delta[i], delta[i] / sigma)
        rows.append(row + "\n")
    return (HEADER if delta is None else HEADER_EXP) + "".join(rows)


def main(argv=None):
    ap = argument_parser()
    ap.add_argument("--probe", type=float, default=1.0, help="probe radius (A), 0 .. 2.0: a parameter of the method")
    ap.add_argument("--cell", type=float, default=0.5, help="lattice step (A), 0.1 .. 2.0")
    ap.add_argument("--experimental", type=float, default=None, help="the measured CCS (A^2): rows by |K CCS_PA - X|")
    ap.add_argument("--sigma", type=float, default=1.0, help="the measurement's standard deviation (A^2)")
    ap.add_argument("--scale", type=float, default=1.0, help="K, the calibration of the projection approximation to the experiment")
    ap.add_argument("--top", type=int, default=0, help="ccs/model_<k>.pdb of the first N rows")
    args = ap.parse_args(argv)
    if not args.sigma > 0.0:
        raise SystemExit("--sigma must be > 0")
    h = int(np.rint(1000.0 * args.cell))

    pkg, setup, sim = open_run(args.setup)
    cx = build_complex(pkg, setup, sim)
    entries = candidates(swarm_list(args.swarms, setup), args.step, args.all)
    poses = pose_matrix(entries, args.step, cx.pose_len)
    got = cx.ccs(poses, 2, args.probe, args.cell, views=True)      # the one GPU call over the candidates
    ms = cx.last_kernel_ms()
    ccs, smallest, largest = areas(got["counts"], h)
    delta = None if args.experimental is None else deltas(ccs, args.experimental, args.scale)
    order = rank_rows(len(entries), delta)

    text = ""
    if len(entries):
        for what, name in ((0, "receptor"), (1, "ligand")):
            try:
                alone = areas(cx.ccs(poses[:1], what, args.probe, args.cell, views=True)["counts"], h)
            except pkg.LightdockError:      # no atom of that side takes part
                continue
            text += monomer_text(name, alone[0][0], alone[1][0], alone[2][0])
    os.makedirs("ccs", exist_ok=True)
    with open(os.path.join("ccs", "rank_ccs.list"), "w") as f:
        f.write(text + rank_text(entries, order, ccs, smallest, largest, delta, args.sigma))
    for k, i in enumerate(order[:max(0, args.top)], 1):
        cx.write_pdb(poses[i], os.path.join("ccs", "model_%d.pdb" % k))
    print("%d models measured (%.3f ms of device work, %d views, cell %.3f A, probe %.3f A)%s"
          % (len(entries), ms, VIEWS, h / 1000.0, args.probe, ": CCS_PA %.1f ... %.1f A^2" % (ccs.min(), ccs.max()) if len(entries) else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
