// anm.hpp -- the host side of K4, normal modes of an anisotropic network model (lightdock_hip.h, "Normal modes"; the
// kernels: kernels/anm.hpp).  What lightdock3_setup.py asks ProDy for and the docking run then reads as rec_nm.npy /
// lig_nm.npy (src/bin/lightdock-rust.rs:216-254): one node a residue, the Hessian of unit springs within a cutoff, the
// modes after the six rigid-body ones, every atom moving with its residue's node.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "host/pdb_file.hpp"

namespace ld {

// The node atom (an index into the file's records) of every residue: its first atom named CA, else its first atom named
// C4'.  Throws LD_ERR_INVALID naming the residue that has neither.
std::vector<uint32_t> anm_node_atoms(const PdbFile &pdb);

struct AnmResult {
    std::vector<double> modes;        // k x n_atoms x 3
    std::vector<double> eigenvalues;  // k, ascending
};

// The modes 7 .. 6 + k of m nodes, spread over n_atoms atoms (node_of_atom; NULL: the nodes themselves, n_atoms = m) and
// normalised over them; rmsd > 0: scaled by the amplitude rule.  Throws before anything runs on the device for arguments
// the header refuses; LD_ERR_INVALID after the solve for a floppy network, LD_ERR_INTERNAL when the sweeps run out.
// The device state lives for the call only, so a call depends on nothing but its arguments.
AnmResult anm_solve(const double *node_xyz, size_t m, size_t k, double cutoff, const uint32_t *node_of_atom, size_t n_atoms,
                    double rmsd);

// The kernels of this thread's last anm_solve that reached the device, in ms (HIP events); 0 before the first.
double anm_last_kernel_ms();

}  // namespace ld
