"""How well every model of a run fits a cryo-EM density map, with ALL candidates in ONE ld_complex_density_fit call on the
GPU (include/lightdock_hip.h, "Density fit": every model's atoms are spread over the map's voxels by an integer table of a
Gaussian at the map's resolution, and the exact sums of that simulated density against the map give the correlations).

    cd run_dir && python lightdock-rust_amd/emfit.py <setup.json> <step> --map MAP.mrc --resolution 10 [--swarms 0-9] [--all]
                                                     [--threshold T] [--shift DX DY DZ] [--bin K] [--top N] [--write-map N]

Candidates as filter.py: the entries run_dir.ranking() forms from swarm_<i>/cluster.repr and gso_<step>.out, or with --all
every glowworm of every selected swarm by scoring.  Each is measured at the full-precision pose of its gso file.

The map is an MRC2014 / CCP4 file, read with numpy alone: the 1024-byte header, modes 0 (int8), 1 (int16), 2 (float32) and
6 (uint16), either byte order as the machine stamp says, nsymbt bytes of extended header skipped, mapc / mapr / maps
permuted to x fastest.  The cell angles must be 90 degrees.  The voxel step is cella / m in whole thousandths of an A; the
origin comes from header words 50-52 when any is non-zero, else nstart x step; --shift (A) is added to it.  The map must be
in the run's frame, that of lightdock_<receptor>.pdb.  Since the step is rounded, the far corner drifts by n x |cella / m -
step|, which the tool prints.  A file whose size does not match its header is refused.  --bin K averages K^3 voxels on
the host (trailing voxels that fill no block are dropped; the origin moves to the block's centre, rounded down to a
thousandth).  Values below --threshold count as no density.

  emfit/rank_emfit.list     per candidate: swarm, glowworm, the gso file's scoring, cc (correlation about zero), ccm
                            (about the means), inside (the share of simulated density in voxels with map density), outside
                            (atoms in no voxel's cell); sorted by ccm descending, ties in the order of the scoring rank;
                            scores with 17 digits
  emfit/model_<k>.pdb       with --top N, the k-th row's model (k = 1 .. N)
  emfit/model_<k>.mrc       with --write-map N, the k-th row's simulated voxels, mode 2, on the map's grid

sigma = rint(225 x resolution) thousandths, which is resolution / (pi sqrt 2).  Path rules as launch.py.
"""
import os
import struct
import sys

import numpy as np

try:
    from .run_dir import argument_parser, build_complex, candidates, open_run, pose_matrix, swarm_list
except ImportError:  # run as a script
    from run_dir import argument_parser, build_complex, candidates, open_run, pose_matrix, swarm_list

HEADER_BYTES = 1024
MODES = {0: "i1", 1: "i2", 2: "f4", 6: "u2"}
HEADER = "Swarm  Glowworm     Scoring                       cc                      ccm                   inside  outside\n"


def read_mrc(path):
    """An MRC2014 / CCP4 file -> (rho (nz, ny, nx) float32, origin (x, y, z), step (x, y, z), drift (x, y, z) in A); origin
    and step in whole thousandths of an A.  ValueError on anything the rule above refuses."""
    raw = open(path, "rb").read()
    if len(raw) < HEADER_BYTES:
        raise ValueError("%s: shorter than an MRC header" % path)
    stamp = raw[212]
    if stamp == 0x44:
        order = "<"
    elif stamp == 0x11:
        order = ">"
    else:
        raise ValueError("%s: machine stamp 0x%02x is neither little- nor big-endian" % (path, stamp))
    words = struct.unpack(order + "10i6f3i3fii", raw[:24 * 4])
    nc, nr, ns, mode = words[0:4]
    nstart, m, cella, cellb, axes = words[4:7], words[7:10], words[10:13], words[13:16], words[16:19]
    nsymbt = words[23]
    file_origin = struct.unpack(order + "3f", raw[49 * 4:52 * 4])
    if mode not in MODES:
        raise ValueError("%s: mode %d is not 0, 1, 2 or 6" % (path, mode))
    if min(nc, nr, ns) < 1 or min(m) < 1 or nsymbt < 0:
        raise ValueError("%s: the header holds a size that is not positive" % path)
    if sorted(axes) != [1, 2, 3]:
        raise ValueError("%s: mapc, mapr, maps are not a permutation of 1, 2, 3" % path)
    if any(abs(a - 90.0) > 1e-3 for a in cellb):
        raise ValueError("%s: cell angles %s are not 90 degrees" % (path, list(cellb)))
    dtype = np.dtype(order + MODES[mode])
    if len(raw) != HEADER_BYTES + nsymbt + nc * nr * ns * dtype.itemsize:
        raise ValueError("%s: %d bytes, the header says %d" % (path, len(raw), HEADER_BYTES + nsymbt + nc * nr * ns * dtype.itemsize))
    data = np.frombuffer(raw, dtype=dtype, offset=HEADER_BYTES + nsymbt).reshape(ns, nr, nc)
    file_axes = [axes[2], axes[1], axes[0]]                              # the space axis of the array's axes 0, 1, 2
    rho = np.ascontiguousarray(np.transpose(data, [file_axes.index(3), file_axes.index(2), file_axes.index(1)]), dtype=np.float32)
    start = [0, 0, 0]
    for k in range(3):
        start[axes[k] - 1] = nstart[k]                                   # nstart is given for columns, rows, sections
    n = rho.shape[::-1]
    spacing = [float(cella[k]) / m[k] for k in range(3)]
    step = [int(np.rint(1000.0 * s)) for s in spacing]
    if any(o != 0.0 for o in file_origin):
        origin = [int(np.rint(1000.0 * float(o))) for o in file_origin]
    else:
        origin = [start[k] * step[k] for k in range(3)]
    drift = [n[k] * abs(spacing[k] - step[k] / 1000.0) for k in range(3)]
    return rho, tuple(origin), tuple(step), tuple(drift)


def write_mrc(path, grid, origin, step):
    """grid (nz, ny, nx) -> an MRC2014 file of mode 2, little-endian, x fastest; origin and step in thousandths."""
    grid = np.ascontiguousarray(grid, dtype="<f4")
    nz, ny, nx = grid.shape
    head = bytearray(HEADER_BYTES)
    struct.pack_into("<10i", head, 0, nx, ny, nz, 2, 0, 0, 0, nx, ny, nz)
    struct.pack_into("<6f", head, 40, nx * step[0] / 1000.0, ny * step[1] / 1000.0, nz * step[2] / 1000.0, 90.0, 90.0, 90.0)
    struct.pack_into("<3i", head, 64, 1, 2, 3)
    struct.pack_into("<3f", head, 76, float(grid.min()), float(grid.max()), float(grid.mean(dtype=np.float64)))
    struct.pack_into("<2i", head, 88, 1, 0)
    struct.pack_into("<3f", head, 196, origin[0] / 1000.0, origin[1] / 1000.0, origin[2] / 1000.0)
    head[208:212] = b"MAP "
    head[212:216] = bytes([0x44, 0x44, 0, 0])
    struct.pack_into("<f", head, 216, float(grid.std(dtype=np.float64)))
    with open(path, "wb") as f:
        f.write(bytes(head))
        f.write(grid.tobytes())


def bin_map(rho, origin, step, k):
    """The mean of every block of k^3 voxels (float64 sums, then float32); voxels that fill no block are dropped."""
    if k == 1:
        return rho, origin, step
    nz, ny, nx = (s // k for s in rho.shape)
    if min(nz, ny, nx) < 1:
        raise ValueError("--bin %d leaves no voxel" % k)
    blocks = rho[:nz * k, :ny * k, :nx * k].astype(np.float64).reshape(nz, k, ny, k, nx, k)
    return (blocks.mean(axis=(1, 3, 5)).astype(np.float32), tuple(o + (k - 1) * s // 2 for o, s in zip(origin, step)),
            tuple(k * s for s in step))


def rank_rows(entries, ccm):
    """Indices of the entries by ccm descending, ties in the entries' own order (the scoring rank)."""
    return sorted(range(len(entries)), key=lambda i: -ccm[i])


def rank_text(entries, order, cc, ccm, inside, outside):
    return HEADER + "".join("%5d %9d %11.5f %24.17g %24.17g %24.17g %8d\n" % (entries[i][0], entries[i][1], entries[i][3]["scoring"], cc[i],
                                                                          ccm[i], inside[i], outside[i]) for i in order)


def main(argv=None):
    ap = argument_parser()
    ap.add_argument("--map", required=True, help="the density map, MRC2014 / CCP4, in the run's frame")
    ap.add_argument("--resolution", type=float, required=True, help="of the map, A")
    ap.add_argument("--threshold", type=float, default=0.0, help="map values below it count as no density")
    ap.add_argument("--shift", type=float, nargs=3, default=(0.0, 0.0, 0.0), metavar=("DX", "DY", "DZ"), help="added to the map's origin (A)")
    ap.add_argument("--bin", type=int, default=1, help="average K^3 voxels before the fit")
    ap.add_argument("--top", type=int, default=0, help="emfit/model_<k>.pdb of the first N rows")
    ap.add_argument("--write-map", type=int, default=0, help="emfit/model_<k>.mrc of the first N rows")
    args = ap.parse_args(argv)
    if args.bin < 1:
        raise SystemExit("--bin must be >= 1")
    map_path = os.path.abspath(args.map)
    try:
        rho, origin, step, drift = read_mrc(map_path)
        rho, origin, step = bin_map(rho, origin, step, args.bin)
    except ValueError as e:
        raise SystemExit(str(e))
    origin = tuple(o + int(np.rint(1000.0 * d)) for o, d in zip(origin, args.shift))
    sigma = int(np.rint(225.0 * args.resolution))
    print("map %d x %d x %d voxels of %.3f x %.3f x %.3f A from (%.3f, %.3f, %.3f); the rounded step drifts %.4f A at the far corner"
          % (rho.shape[2], rho.shape[1], rho.shape[0], step[0] / 1000.0, step[1] / 1000.0, step[2] / 1000.0, origin[0] / 1000.0,
             origin[1] / 1000.0, origin[2] / 1000.0, max(drift)))

    pkg, setup, sim = open_run(args.setup)
    cx = build_complex(pkg, setup, sim)
    entries = candidates(swarm_list(args.swarms, setup), args.step, args.all)
    poses = pose_matrix(entries, args.step, cx.pose_len)
    try:
        density = pkg.Density(rho, origin, step, args.threshold)
        sums = cx.density_fit(poses, density, sigma)                      # the one GPU call
    except pkg.LightdockError as e:
        if "wider than 16 voxels" in str(e):
            raise SystemExit("%s (try --bin %d)" % (e, args.bin + 1))
        raise
    ms = cx.last_kernel_ms()
    cc, ccm, inside = pkg.density_scores(density, sums)
    order = rank_rows(entries, ccm)

    os.makedirs("emfit", exist_ok=True)
    with open(os.path.join("emfit", "rank_emfit.list"), "w") as f:
        f.write(rank_text(entries, order, cc, ccm, inside, sums["outside"]))
    for k, i in enumerate(order[:max(0, args.top)], 1):
        cx.write_pdb(poses[i], os.path.join("emfit", "model_%d.pdb" % k))
    chosen = order[:max(0, args.write_map)]
    if chosen:
        grids = cx.simulate_density(poses[chosen], density, sigma)
        for k, grid in enumerate(grids, 1):
            write_mrc(os.path.join("emfit", "model_%d.mrc" % k), grid, origin, step)
    print("%d models fitted at %.1f A, sigma %.3f A (%.3f ms of device work)%s"
          % (len(entries), args.resolution, sigma / 1000.0, ms, ": ccm %.4f ... %.4f" % (ccm[order[0]], ccm[order[-1]]) if order else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
