// pose_energy_tail.hpp -- the tail of a pose's energy (device code): the score of the pair sums, the restraint terms and the
// membrane penalty (src/dfire.rs:347-361, src/dna.rs:513-514, src/scoring.rs:21-47).  ONE copy of the reference's formula for
// the kernels that finish a pose: pose_energy_finish (pose_energy.hip) and dfire_bm_finish (dfire_bm.hip).
#pragma once

#include "pose_energy.hpp"

namespace ld {

// Eight lanes per pose in the finishing kernels: they share the partial sums and the membrane scan, lane 0 applies the tail.
constexpr int kFinishLanes = 8;

__device__ __forceinline__ bool flag_set(const uint32_t *words, uint32_t slot) {
    return (words[slot >> 5] >> (slot & 31)) & 1u;
}

// scoring.rs:21-36 over flag slots
__device__ inline double satisfied_fraction(const uint32_t *words, int n_groups, const uint32_t *offsets,
                                            const uint32_t *slots) {
    if (n_groups == 0) return 0.0;
    int hit = 0;
    for (int g = 0; g < n_groups; g++) {
        for (uint32_t k = offsets[g]; k < offsets[g + 1]; k++)
            if (flag_set(words, slots[k])) {
                hit++;
                break;
            }
    }
    return (double)hit / (double)n_groups;
}

// membrane beads (src/scoring.rs:38-47) whose flag is set: the pose's eight lanes share the scan (lane `sub` takes the beads
// sub, sub + 8, ...), the count is an integer.  Every lane of the wave calls this (the shuffles); a lane that is not `live`
// brings zero.  The slots of four trips are loaded before their flag words: two dependent round trips instead of eight.
__device__ __forceinline__ int membrane_beads(const uint32_t *rwords, int n_membrane, const uint32_t *membrane_slots, int sub, bool live) {
    int beads = 0;
    if (live) {
        int k = sub;
        for (; k + 3 * kFinishLanes < n_membrane; k += 4 * kFinishLanes) {
            const uint32_t a = membrane_slots[k], b = membrane_slots[k + kFinishLanes], c = membrane_slots[k + 2 * kFinishLanes],
                           d = membrane_slots[k + 3 * kFinishLanes];
            const uint32_t wa = rwords[a >> 5], wb = rwords[b >> 5], wc = rwords[c >> 5], wd = rwords[d >> 5];
            beads += (int)(((wa >> (a & 31)) & 1u) + ((wb >> (b & 31)) & 1u) + ((wc >> (c & 31)) & 1u) + ((wd >> (d & 31)) & 1u));
        }
        for (; k < n_membrane; k += kFinishLanes) beads += flag_set(rwords, membrane_slots[k]) ? 1 : 0;
    }
    if (n_membrane > 0)
        for (int d = 1; d < kFinishLanes; d <<= 1) beads += __shfl_xor(beads, d);
    return beads;
}

// The energy of one pose from its pair sums (DFIRE: s0 = the table sum; DNA: s0 = electrostatics, s1 = van der Waals), its flag
// words (receptor's, then ligand's) and its count of flagged membrane beads.
__device__ __forceinline__ double pose_energy_tail(int method, double s0, double s1, const uint32_t *rwords, int rec_flag_words,
                                                   const TailTables &tail, int beads) {
    double score;
    if (method == 0) {
        score = (s0 * 0.0157 - 4.7) * -1.0;  // src/dfire.rs:347
    } else {
        const double total_elec = s0 * 332.0 / 4.0;  // src/dna.rs:513
        score = (total_elec + s1) * -1.0;            // src/dna.rs:514
    }
    const uint32_t *lwords = rwords + rec_flag_words;
    const double pr = satisfied_fraction(rwords, tail.n_rec_groups, tail.rec_group_offsets, tail.rec_group_slots);
    const double pl = satisfied_fraction(lwords, tail.n_lig_groups, tail.lig_group_offsets, tail.lig_group_slots);
    double penalty = 0.0;
    if (tail.n_membrane > 0) {  // src/scoring.rs:38-47, src/dfire.rs:355-359
        const double intersection = (double)beads / (double)tail.n_membrane;
        if (intersection > 0.0) penalty = 999.0 * intersection;
    }
    return score + pr * score + pl * score - penalty;  // src/dfire.rs:361
}

}  // namespace ld
