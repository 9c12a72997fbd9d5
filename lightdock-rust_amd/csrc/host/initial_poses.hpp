// initial_poses.hpp -- the start poses of a swarm's glowworms (lightdock_hip.h, "Preparing a run", rule 5), host only:
// what lightdock3_setup.py writes into init/initial_positions_<i>.dat, by a rule of this project's own on the StdRng
// stream of ld_stdrng_key.  Counter based: row (swarm, glowworm) reads its own draws, so it is the same bits alone or in
// a batch.  This file is compiled with -ffp-contract=off like everything else; the rule is stated operation by operation.
#pragma once

#include <cstddef>
#include <cstdint>

namespace ld {

constexpr int kPoseDrawShift = 16;   // glowworm g of swarm s reads draws ((s G + g) << 16) + j

// The 16 words of ChaCha20 block `counter` under `key` (rand_chacha 0.2: a 64-bit counter in words 12-13, stream id 0):
// what kernels/gso_step.hip computes on the device.
void chacha20_block(const uint32_t key[8], uint64_t counter, uint32_t out[16]);

struct PoseRequest {
    uint64_t seed = 0;
    size_t glowworms = 0;       // G of the run: the stride of the draw numbers
    size_t swarm = 0;           // s
    size_t first = 0, n = 0;    // rows g = first .. first + n - 1
    double centre[3] = {0, 0, 0};
    double radius = 10.0;
    const double *rec_points = nullptr;  // n_rec x 3: the atom of every receptor restraint residue
    size_t n_rec = 0;
    const double *lig_points = nullptr;  // n_lig x 3: ... of every ligand restraint residue, in the centred ligand frame
    size_t n_lig = 0;
    size_t anm_rec = 0, anm_lig = 0;
};

// rows: n x (7 + anm_rec + anm_lig); draws: n counts of u64 draws consumed, or NULL.  Throws LD_ERR_INVALID before anything
// is written.
void initial_poses(const PoseRequest &r, double *rows, uint64_t *draws);

}  // namespace ld
