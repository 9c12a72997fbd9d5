// prepare.hpp -- the host side of K5, the swarm centres of a run (lightdock_hip.h, "Preparing a run"; the kernels:
// kernels/swarm_shell.hpp): what lightdock3_setup.py computes before a run, as an integer rule of this project's own on the
// thousandths "%8.3f" prints.  The three calls check their arguments before anything runs on the device, own their device
// memory for the call only, and leave every output untouched when they refuse.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace ld {

// max over i, j of |x_i - x_j|^2 of n >= 1 points (n x 3 thousandths, |x| <= 2 000 000).
uint64_t swarm_diameter2(const int32_t *xyz, size_t n);

struct SwarmShell {
    uint64_t nodes = 0;               // lattice nodes tested
    std::vector<int32_t> candidates;  // count x 3, lexicographic
};
// The shell candidates of n atoms (atoms: n x 4, x y z E; bead: n flags or NULL) on a lattice of spacing h.
SwarmShell swarm_shell(const int32_t *atoms, const uint8_t *bead, size_t n, int32_t spacing);

struct SwarmCentres {
    std::vector<uint32_t> index;  // into the points, in the order picked
    std::vector<uint64_t> gap2;   // the value each was picked at: |p|^2 for the first, its gap^2 for the others
};
// Farthest-point sampling of n points (n x 3): at most max_centres, and with cover > 0 no centre whose gap^2 <= cover^2.
SwarmCentres swarm_centres(const int32_t *points, size_t n, size_t max_centres, int32_t cover);

// The kernels of this thread's last call of the three that reached the device, in ms (HIP events); 0 before the first.
double setup_last_kernel_ms();

}  // namespace ld
