"""How well every model of a run fits an experimental SAXS curve, with ALL candidates in ONE ld_complex_saxs call on the GPU
(include/lightdock_hip.h, "Small-angle scattering": the exact histogram of pair distances on the integer thousandths
"%8.3f" prints, by pair class, and the Debye sum over it; the profile is "vacuum minus excluded volume" of the atoms in
the files -- no implicit hydrogens, no hydration layer).

    cd run_dir && python lightdock-rust_amd/saxs.py <setup.json> <step> --curve exp.dat [--swarms 0-9] [--all]
                                                    [--qmax 0.5] [--unit A|nm] [--width 0.5] [--profiles N]

Candidates as filter.py: the entries run_dir.ranking() forms from swarm_<i>/cluster.repr and gso_<step>.out, or with --all
every glowworm of every selected swarm by scoring.  Each is measured at the full-precision pose of its gso file.

The curve file holds lines of "q I sigma"; lines that start with # and blank lines are skipped, anything else that is not
three numbers is an error.  q must ascend strictly; points above --qmax are dropped; --unit nm divides q by 10.

  saxs/rank_saxs.list       per candidate: swarm, glowworm, the gso file's scoring, chi2 and scale of the fit, the radius
                            of gyration and the largest distance (A) of the atoms that take part; sorted by chi2
                            ascending, ties in the order of the scoring rank
  saxs/profile_<k>.dat      with --profiles N, for the k-th row (k = 1 .. N): q, I_exp, sigma, scale x I

The bin count comes from a bound on the largest distance of a model; if the library still reports a pair beyond the last
bin, the bound is doubled and the call repeated once.  At most 1024 bins: a bound they cannot hold at --width raises the
width, and the tool says so.  Path rules as launch.py.
"""
import math
import os
import sys

import numpy as np

try:
    from .run_dir import argument_parser, build_complex, candidates, open_run, pose_matrix, swarm_list
except ImportError:  # run as a script
    from run_dir import argument_parser, build_complex, candidates, open_run, pose_matrix, swarm_list

MAX_BINS, MAX_Q = 1024, 1024
MIN_WIDTH, MAX_WIDTH = 100, 2000   # thousandths
MODE_MARGIN = 10.0                 # A: what the modes may add to a model's extent
HEADER = "Swarm  Glowworm     Scoring          chi2         scale        Rg      Dmax\n"


def parse_curve(text, qmax=0.5, unit="A"):
    """The text of a curve file -> (q in 1 / A, I, sigma) as arrays.  ValueError on anything the rule above refuses."""
    if unit not in ("A", "nm"):
        raise ValueError('unit must be "A" or "nm"')
    rows = []
    for number, line in enumerate(text.splitlines(), 1):
        if not line.strip() or line.lstrip().startswith("#"):
            continue
        fields = line.split()
        try:
            if len(fields) != 3:
                raise ValueError
            q, i, sigma = (float(v) for v in fields)
        except ValueError:
            raise ValueError("line %d is not 'q I sigma': %r" % (number, line)) from None
        if not all(math.isfinite(v) for v in (q, i, sigma)):
            raise ValueError("line %d holds a value that is not finite" % number)
        if unit == "nm":
            q = q / 10.0
        if q < 0.0:
            raise ValueError("line %d: q is negative" % number)
        if sigma <= 0.0:
            raise ValueError("line %d: sigma must be > 0" % number)
        if rows and q <= rows[-1][0]:
            raise ValueError("line %d: q does not ascend" % number)
        rows.append((q, i, sigma))
    rows = [r for r in rows if r[0] <= qmax]
    if not rows:
        raise ValueError("the curve holds no point up to qmax = %g / A" % qmax)
    if len(rows) > MAX_Q:
        raise ValueError("the curve holds %d points up to qmax, at most %d are taken" % (len(rows), MAX_Q))
    a = np.array(rows, dtype=np.float64)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()


def bin_plan(bound, width):
    """bound (A) on the largest distance and the width asked for (thousandths) -> (width, bins): the bins that hold the
    bound, at most MAX_BINS; the width is raised when they cannot."""
    reach = int(math.ceil(bound * 1000.0)) + 1
    bins = (reach + width - 1) // width
    if bins > MAX_BINS:
        width = (reach + MAX_BINS - 1) // MAX_BINS
        bins = (reach + width - 1) // width
    if width > MAX_WIDTH:
        raise ValueError("a largest distance of %.1f A does not fit %d bins of at most %.1f A" % (bound, MAX_BINS, MAX_WIDTH / 1000.0))
    return width, max(1, bins)


def size_measures(counts, width, n_part):
    """counts (21, bins) of one pose -> (Rg, Dmax) in A: Rg^2 = sum_k H_k r_k^2 / n^2 with H_k the pairs of bin k over all
    pair classes and r_k = (k + 0.5) w; Dmax is the upper edge of the last bin that holds a pair (0 without pairs)."""
    H = np.asarray(counts, dtype=np.float64).sum(axis=0)
    r = (np.arange(H.size) + 0.5) * width / 1000.0
    filled = np.flatnonzero(H)
    rg = math.sqrt(float((H * r * r).sum()) / float(n_part) ** 2) if n_part else 0.0
    return rg, (float(filled[-1] + 1) * width / 1000.0 if filled.size else 0.0)


def rank_rows(entries, chi2):
    """Indices of the entries by chi2 ascending, ties in the entries' own order (the scoring rank)."""
    return sorted(range(len(entries)), key=lambda i: chi2[i])


def rank_text(entries, order, chi2, scale, measures):
    return HEADER + "".join("%5d %9d %11.5f %13.6e %13.6e %9.3f %9.3f\n" % (entries[i][0], entries[i][1], entries[i][3]["scoring"], chi2[i],
                                                                       scale[i], measures[i][0], measures[i][1]) for i in order)


def profile_text(q, i_exp, sigma, model):
    return "".join("%.8e %.8e %.8e %.8e\n" % row for row in zip(q, i_exp, sigma, model))


def file_radius(path):
    """The largest distance of an ATOM / HETATM record of the file from the origin of its frame (A)."""
    xyz = [[float(line[30:38]), float(line[38:46]), float(line[46:54])] for line in open(path) if line.startswith(("ATOM  ", "HETATM"))]
    return float(np.sqrt((np.array(xyz).reshape(-1, 3) ** 2).sum(axis=1)).max()) if xyz else 0.0


def distance_bound(rec_radius, lig_radius, poses):
    """No two atoms of a posed model are farther apart: two of one molecule, or one of each across the translation."""
    shift = float(np.sqrt((poses[:, :3] ** 2).sum(axis=1)).max()) if len(poses) else 0.0
    return max(2.0 * rec_radius, 2.0 * lig_radius, rec_radius + lig_radius + shift) + MODE_MARGIN


def main(argv=None):
    ap = argument_parser()
    ap.add_argument("--curve", required=True, help="the experimental curve: lines of q I sigma")
    ap.add_argument("--qmax", type=float, default=0.5, help="points above it are dropped (1 / A)")
    ap.add_argument("--unit", choices=("A", "nm"), default="A", help="the unit of 1 / q in the curve file")
    ap.add_argument("--width", type=float, default=0.5, help="bin width (A), 0.1 .. 2.0")
    ap.add_argument("--profiles", type=int, default=0, help="saxs/profile_<k>.dat of the first N rows")
    args = ap.parse_args(argv)
    q, i_exp, sigma = parse_curve(open(args.curve).read(), args.qmax, args.unit)
    width = int(round(1000.0 * args.width))
    if not MIN_WIDTH <= width <= MAX_WIDTH:
        raise SystemExit("--width must be 0.1 .. 2.0 A")

    pkg, setup, sim = open_run(args.setup)
    cx = build_complex(pkg, setup, sim)
    entries = candidates(swarm_list(args.swarms, setup), args.step, args.all)
    poses = pose_matrix(entries, args.step, cx.pose_len)
    classes = np.concatenate([cx.saxs_classes(0), cx.saxs_classes(1)])
    n_part, left_out = int((classes != 255).sum()), int((classes == 255).sum())
    bound = distance_bound(file_radius(os.path.join(sim, "lightdock_" + setup["receptor_pdb"])),
                           file_radius(os.path.join(sim, "lightdock_" + setup["ligand_pdb"])), poses)
    for attempt in (0, 1):
        w, bins = bin_plan(bound, width)
        if w != width:
            print("bin width raised from %.3f to %.3f A: %d bins hold %.1f A" % (width / 1000.0, w / 1000.0, bins, bound))
        try:
            intensity, counts = cx.saxs(poses, q, w / 1000.0, bins, counts=True)      # the one GPU call
            break
        except pkg.LightdockError as e:
            if attempt or "beyond the last bin" not in str(e):
                raise
            bound *= 2.0
    ms = cx.last_kernel_ms()
    scale, chi2 = pkg.saxs_fit(intensity, i_exp, sigma)
    measures = [size_measures(c, w, n_part) for c in counts]
    order = rank_rows(entries, chi2)

    os.makedirs("saxs", exist_ok=True)
    with open(os.path.join("saxs", "rank_saxs.list"), "w") as f:
        f.write(rank_text(entries, order, chi2, scale, measures))
    for k, i in enumerate(order[:max(0, args.profiles)], 1):
        with open(os.path.join("saxs", "profile_%d.dat" % k), "w") as f:
            f.write(profile_text(q, i_exp, sigma, scale[i] * intensity[i]))
    print("%d models fitted to %d points (%.3f ms of device work, %d bins of %.3f A); %d atoms take part, %d do not%s"
          % (len(entries), len(q), ms, bins, w / 1000.0, n_part, left_out,
             ": chi2 %.4g ... %.4g" % (chi2[order[0]], chi2[order[-1]]) if order else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
