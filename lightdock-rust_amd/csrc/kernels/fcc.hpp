// fcc.hpp -- launch interface of K3g, clustering by the fraction of common contacts (kernels/fcc.hip; DESIGN §5 K3g;
// lightdock_hip.h, "Clustering by common contacts"): what the host side (fcc.cpp) and the kernels share, and the neighbour
// test, which is host code too so that a CPU build can check it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels/cluster.hpp"

namespace ld {

constexpr int kPairThreads = 512;
constexpr int kPairSlots = 1024;                   // as kContactSlots
constexpr size_t kFccMaxPoses = size_t(1) << 22;   // ld_complex_pair_contacts: poses a call
constexpr size_t kFccMaxSets = 65536;              // clustering: the neighbour bits, n^2 / 8 B, stay within 512 MiB
constexpr size_t kFccMaxCommonSets = 16384;        // ld_fcc_common: the n x n words stay within 1 GiB
constexpr size_t kFccMaxRowBytes = size_t(1) << 30;  // the bit rows, n x ceil(U / 32) words
constexpr int kFccTile = 64;                       // poses a side of a tile of fcc_common
constexpr int kFccChunkWords = 32;                 // words of every row of a tile staged in LDS at a time
constexpr int kFccLdsStride = kFccTile + 4;        // a word column of a staged tile: 16-B aligned, staging stores 4-way at worst
constexpr int kFccCommonThreads = 256;             // 16 x 16 threads, 4 x 4 pairs each
constexpr int kFccGreedyThreads = 1024;
constexpr int kFccScanThreads = 1024;
constexpr int kFccRankWords = 32;                  // words of the presence bitmap between two stored ranks (1024 keys)

// i != j is the caller's: poses i and j are neighbours iff both sets are non-empty and 1000 c >= T max(s_i, s_j).
__host__ __device__ inline bool fcc_neighbours(uint32_t c, uint32_t si, uint32_t sj, uint32_t T) {
    const uint32_t larger = si > sj ? si : sj;
    return si > 0 && sj > 0 && 1000ull * c >= (unsigned long long)T * larger;
}

// The words the host reads back between launches.
struct FccStatus {
    unsigned long long total;  // fcc_exclusive_scan: the sum of its input
    uint32_t n_clusters;       // fcc_greedy
    uint32_t rounds;           // fcc_greedy: centres picked one at a time (the singletons of the tail are not rounds)
};

// The pair sets of n poses, in two launches of the same pyramid as complex_contacts (residue boxes, ligand groups, 8 x 8 atom
// walks): a workgroup marks the touching residue pairs of a pose in its slot's bitmap, bit (r, l) at word r * lw + (l >> 5)
// with lw = ceil(n_lig_res / 32), and then either counts them (offsets == nullptr: counts[pose]) or emits their keys
// r * n_lig_res + l in ascending order at keys[offsets[pose]].  A set is a bitmap first, so no order depends on a schedule.
// `slots` workgroups; atoms_ws: slots x d.n_atoms int4; boxes_ws: slots x 6 x d.n_boxes() ints, not read with d.boxes_in_lds;
// pairs_ws: slots x d.n_rec_res x lw words; overflow: one int.
hipError_t launch_complex_pair_sets(const ComplexDevice &m, const ContactsDevice &d, const double *poses, size_t stride, size_t n,
                                    uint32_t C2, size_t slots, int4 *atoms_ws, int *boxes_ws, uint32_t *pairs_ws,
                                    const uint32_t *offsets, uint32_t *counts, uint32_t *keys, int *overflow, hipStream_t stream);
// One workgroup.  out: n + 1 words, out[i] = in[0] + ... + in[i - 1] (mod 2^32); *total: the whole sum.  out may be `in`.
hipError_t launch_fcc_exclusive_scan(const uint32_t *in, size_t n, uint32_t *out, unsigned long long *total, hipStream_t stream);

// The dense renumbering of the union of all keys.  bitmap: n_rank x kFccRankWords words, cleared by the caller, bit
// key - key_lo; rank: n_rank + 1 words.
hipError_t launch_fcc_mark(const uint32_t *keys, size_t total, uint32_t key_lo, uint32_t *bitmap, hipStream_t stream);
hipError_t launch_fcc_rank_counts(const uint32_t *bitmap, size_t n_rank, uint32_t *rank, hipStream_t stream);
// A wave a set.  The column of key k is the number of marked keys below it: rank (scanned) and the bitmap give it.
// row_of: the row of every set, or nullptr for its own index; rows: n x W words and freq: U words, both cleared by the
// caller; cols: a column a key; sizes: by ROW.
hipError_t launch_fcc_rows(const uint32_t *offsets, const uint32_t *keys, size_t n, const uint32_t *row_of, uint32_t key_lo,
                           const uint32_t *bitmap, const uint32_t *rank, size_t W, uint32_t *rows, uint32_t *cols,
                           uint32_t *freq, uint32_t *sizes, hipStream_t stream);
// c_ij = popcount(row_i & row_j) in tiles of kFccTile x kFccTile rows, the upper triangle only; every output word is stored
// once, by the tile that owns it or its mirror image.  nbr (n x NW words, NW = ceil(n / 32)): the neighbour bits of
// fcc_neighbours, both halves; or common (n x n words): c itself, both halves, the diagonal s_i.  Exactly one is non-null.
hipError_t launch_fcc_common(const uint32_t *rows, size_t W, size_t n, const uint32_t *sizes, uint32_t T, uint32_t *nbr,
                             uint32_t *common, hipStream_t stream);
// deg[i] = 1 + popcount(row i of nbr).
hipError_t launch_fcc_degrees(const uint32_t *nbr, size_t n, int *deg, hipStream_t stream);
// One workgroup, every round inside it; rows are taken by (deg descending, row ascending), so the caller's rows are in
// (scoring descending, index ascending) order.  members: n ints of scratch; cluster_of, centres: n each, by row.
hipError_t launch_fcc_greedy(const uint32_t *nbr, size_t n, int *deg, uint32_t min_size, int *members, int32_t *cluster_of,
                             int32_t *centres, FccStatus *status, hipStream_t stream);
// A wave a set: consensus[i] = sum of freq over the set's columns.
hipError_t launch_fcc_consensus(const uint32_t *offsets, const uint32_t *cols, const uint32_t *freq, size_t n,
                                unsigned long long *consensus, hipStream_t stream);

}  // namespace ld
