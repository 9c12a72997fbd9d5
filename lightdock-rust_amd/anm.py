"""Normal modes of a run's two molecules on the GPU: what lightdock3_setup.py asks ProDy for, so that a run with
`use_anm: true` can be prepared from its two PDB files alone.

    cd run_dir && python lightdock-rust_amd/anm.py <setup.json> [--rmsd] [--cutoff 15] [--force]

Reads anm_rec / anm_lig and the two lightdock_* PDB files of the setup (next to setup.json) and writes, into the CWD,
lightdock_rec.nm.npy / lightdock_lig.nm.npy of shape (modes, atoms, 3) and the flattened 1-D <f8 rec_nm.npy / lig_nm.npy
the reference binary reads (lgd_flatten.py's C-order flattening; src/bin/lightdock-rust.rs:216-254).  A side with no modes
in the setup is left out.  Refuses to overwrite any of them without --force, before anything is computed.  Unit modes by
default; --rmsd scales mode k by the setup's anm_rec_rmsd / anm_lig_rmsd with this project's own amplitude rule
(include/lightdock_hip.h, "Normal modes"): the directions are ProDy's, the amplitudes are not those of a setup made with
anm_seed.  Path rules as launch.py.
"""
import argparse
import os
import sys

import numpy as np

try:
    from .run_dir import open_run
except ImportError:  # run as a script
    from run_dir import open_run

SIDES = (("rec", "receptor_pdb"), ("lig", "ligand_pdb"))


def outputs(side):
    """(shaped file, flattened file) of one side, in the CWD."""
    return "lightdock_%s.nm.npy" % side, "%s_nm.npy" % side


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("setup")
    ap.add_argument("--rmsd", action="store_true", help="scale the modes by anm_rec_rmsd / anm_lig_rmsd of the setup")
    ap.add_argument("--cutoff", type=float, default=15.0, help="spring cutoff between nodes (A)")
    ap.add_argument("--force", action="store_true", help="overwrite mode files that exist")
    args = ap.parse_args(argv)

    pkg, setup, sim = open_run(args.setup)
    sides = [(side, os.path.join(sim, "lightdock_" + setup[key]), int(setup["anm_" + side])) for side, key in SIDES]
    sides = [s for s in sides if s[2] > 0]
    existing = [p for side, _, _ in sides for p in outputs(side) if os.path.exists(p)]
    if existing and not args.force:
        print("anm.py: %s exist%s; --force overwrites" % (", ".join(existing), "s" if len(existing) == 1 else ""), file=sys.stderr)
        return 1
    for side, pdb, k in sides:
        rmsd = float(setup.get("anm_%s_rmsd" % side) or 0.0) if args.rmsd else 0.0
        eig, modes = pkg.anm_modes(pdb, k, cutoff=args.cutoff, rmsd=rmsd)
        shaped, flat = outputs(side)
        np.save(shaped, modes.astype("<f8"))
        np.save(flat, modes.astype("<f8").reshape(-1))
        print("%s: %d modes of %d atoms, eigenvalues %.6g .. %.6g, %.1f ms on the device -> %s, %s" %
              (os.path.basename(pdb), k, modes.shape[1], eig[0], eig[-1], pkg.anm_last_kernel_ms(), shaped, flat))
    return 0


if __name__ == "__main__":
    sys.exit(main())
