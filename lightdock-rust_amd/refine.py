"""Local refinement of the ranked models of a run: every candidate walked uphill to the optimum the swarm left it near, under
the run's own scoring function, with ALL candidates in ONE ld_scorer_refine call on the GPU (include/lightdock_hip.h, "Local
refinement": a compass search over translation, rotation and ANM extents whose every decision is a stated rule).

    cd run_dir && python lightdock-rust_amd/refine.py <setup.json> <step> <dfire|dna|pydock> [--swarms 0-9] [--all] [--top N]
        [--iterations 20] [--trans 1.0] [--rot 0.1] [--nm 0.5] [--halvings 4] [--pdb N]

The scorer is built as launch.py builds it.  Candidates as decompose.py: the entries run_dir.ranking() forms from
swarm_<i>/cluster.repr and gso_<step>.out, or with --all every glowworm of every selected swarm by scoring; --top N keeps the
first N.  Each starts from the full-precision pose of its gso file.  The default steps (1.0 A, 0.1 rad, 0.5 extent units,
halved at most 4 times, 20 iterations) are this project's own; LightDock's -min uses Powell's method instead.

  refined/refined.list              per candidate, sorted by the refined energy, highest first: swarm, glowworm, the gso
                                    file's scoring, the energy before and after, accepted moves, halvings, energy
                                    evaluations, the distance moved (A) and the angle turned (rad, 2 acos |q0 . q1| over the
                                    norms)
  refined/swarm_<i>/gso_<step>.out  that swarm's file with the refined candidates' pose and scoring replaced (17 significant
                                    digits: read_gso gives back the refined doubles) and every other row and column kept, so
                                    the other tools run on the refined models from inside refined/ with --all
  refined/top_<k>.pdb               with --pdb N: the N best refined models (ld_complex_write_pdb)

Path rules as launch.py.
"""
import math
import os
import sys

import numpy as np

try:
    from .run_dir import argument_parser, build_complex, build_scorer, candidates, open_run, pose_matrix, swarm_list
except ImportError:  # run as a script
    from run_dir import argument_parser, build_complex, build_scorer, candidates, open_run, pose_matrix, swarm_list

REFINED_HEADER = "Swarm Glowworm Scoring Before After Accepted Halvings Evaluations Moved Turned\n"


def moved(before, after):
    """Distance between the translations of two poses."""
    d = np.asarray(after[:3], dtype=np.float64) - np.asarray(before[:3], dtype=np.float64)
    return float(np.sqrt(np.dot(d, d)))


def turned(before, after):
    """Angle between the rotations of two poses: 2 acos |q0 . q1| over the norms (the trial quaternions are not normalised)."""
    q0, q1 = np.asarray(before[3:7], dtype=np.float64), np.asarray(after[3:7], dtype=np.float64)
    norms = math.sqrt(float(np.dot(q0, q0))) * math.sqrt(float(np.dot(q1, q1)))
    if not norms > 0.0:
        return float("nan")
    return 2.0 * math.acos(min(1.0, abs(float(np.dot(q0, q1))) / norms))


def refined_rows(entries, poses, refined, stats):
    """One row of refined.list per candidate, sorted by the refined energy, highest first (ties in candidate order)."""
    rows = [(e[0], e[1], e[3]["scoring"], stats["energy_before"][i], stats["energy_after"][i], int(stats["accepted"][i]),
             int(stats["halvings"][i]), int(stats["evaluations"][i]), moved(poses[i], refined[i]), turned(poses[i], refined[i]), i)
            for i, e in enumerate(entries)]
    return sorted(rows, key=lambda r: (-r[4] if r[4] == r[4] else math.inf, r[10]))


def refined_text(rows):
    return REFINED_HEADER + "".join("%5d %5d %12.5f %24.17g %24.17g %5d %5d %8d %10.5f %10.6f\n" % r[:10] for r in rows)


def parse_list(text):
    """A list written above -> (header columns, rows of strings)."""
    lines = text.splitlines()
    return lines[0].split(), [line.split() for line in lines[1:] if line.strip()]


def rewrite_gso(text, refined):
    """The text of a gso file with the rows of `refined` ({glowworm: (pose, energy)}) given that pose in their first
    len(pose) coordinates and that energy as their scoring, both with 17 significant digits.  Everything else -- the
    header, the other rows, a row's further coordinates and its other columns -- keeps its bytes."""
    out, g = [], 0
    for line in text.splitlines(keepends=True):
        if not line.startswith("("):
            out.append(line)
            continue
        if g in refined:
            pose, energy = refined[g]
            inner, rest = line[1:].split(")", 1)
            fields = inner.split(",")
            if len(fields) < len(pose):
                raise ValueError("glowworm %d holds %d coordinates, the refined pose %d" % (g, len(fields), len(pose)))
            head = ", ".join("%.17g" % v for v in pose)
            tail = ",".join(fields[len(pose):])
            body = rest.rstrip("\n")
            end = rest[len(body):]
            cut = len(body.rstrip()) - len(body.rstrip().split()[-1])   # where the last column, the scoring, starts
            line = "(" + head + ("," + tail if tail else "") + ")" + body[:cut] + "%.17g" % energy + end
        out.append(line)
        g += 1
    missing = [k for k in refined if not 0 <= k < g]
    if missing:
        raise ValueError("no glowworm %s in a file of %d" % (missing, g))
    return "".join(out)


def main(argv=None):
    ap = argument_parser()
    ap.add_argument("method")
    ap.add_argument("--top", type=int, default=None, help="only the first N candidates")
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--trans", type=float, default=1.0, help="translation step (A)")
    ap.add_argument("--rot", type=float, default=0.1, help="rotation step (rad)")
    ap.add_argument("--nm", type=float, default=0.5, help="ANM extent step")
    ap.add_argument("--halvings", type=int, default=4, help="times a pose's steps may halve before it is frozen")
    ap.add_argument("--pdb", type=int, default=0, help="write the N best refined models as refined/top_<k>.pdb")
    args = ap.parse_args(argv)

    pkg, setup, sim = open_run(args.setup)
    method = args.method.lower()
    scorer = build_scorer(pkg, setup, sim, method)
    swarms = swarm_list(args.swarms, setup)
    entries = candidates(swarms, args.step, args.all)
    if args.top is not None:
        entries = entries[:max(0, args.top)]
    poses = pose_matrix(entries, args.step, scorer.pose_len)
    out = scorer.refine(poses, iterations=args.iterations, trans_step=args.trans, rot_step=args.rot, nm_step=args.nm,
                        max_halvings=args.halvings)
    rows = refined_rows(entries, poses, out["poses"], out["stats"])

    os.makedirs("refined", exist_ok=True)
    with open(os.path.join("refined", "refined.list"), "w") as f:
        f.write(refined_text(rows))
    for s in swarms:
        mine = {e[1]: (out["poses"][i], out["stats"]["energy_after"][i]) for i, e in enumerate(entries) if e[0] == s}
        os.makedirs(os.path.join("refined", "swarm_%d" % s), exist_ok=True)
        text = open(os.path.join("swarm_%d" % s, "gso_%d.out" % args.step)).read()
        with open(os.path.join("refined", "swarm_%d" % s, "gso_%d.out" % args.step), "w") as f:
            f.write(rewrite_gso(text, mine))
    if args.pdb > 0 and rows:
        cx = build_complex(pkg, setup, sim)
        for k, r in enumerate(rows[:args.pdb], 1):
            cx.write_pdb(out["poses"][r[10]][:cx.pose_len], os.path.join("refined", "top_%d.pdb" % k))
    info = scorer.refine_info()
    print("%d models refined, %d improved (%d energy evaluations, %.3f ms on the device)"
          % (len(entries), int(np.sum(out["stats"]["accepted"] > 0)), info["evaluations"], info["last_kernel_ms"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
