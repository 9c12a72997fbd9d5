// cluster.hpp -- launch interface of K3, the analysis half of a run (kernels/cluster.hip): what the host
// side (complex.cpp) and the kernels share.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace ld {

constexpr int kMaxGlowworms = 4096;  // ld_gso_create's limit; the sort keys of a swarm fill 48 KiB of LDS
constexpr int kBsasThreads = 256;
constexpr int kPoseThreads = 256;
constexpr size_t kClusterWorkspaceBytes = size_t(256) << 20;

constexpr int kContactThreads = 512;
constexpr int kContactSlots = 1024;            // 256 CUs x 4 resident workgroups
constexpr int kResGroup = 8;
constexpr size_t kMaxContactWords = 16384;     // bit words of both sides, kept in LDS (64 KiB: 524 288 residues)
constexpr size_t kMaxBoxLdsBytes = 40 << 10;   // 24 B a box: up to 1706 residues + ligand groups (1k4c: 1327) keep four workgroups a CU

struct ComplexDevice {
    int n_rec = 0, n_lig = 0, anm_rec = 0, anm_lig = 0;
    const double *rec_xyz = nullptr, *lig_xyz = nullptr;      // n x 3, file order
    const double *rec_modes = nullptr, *lig_modes = nullptr;  // anm x n x 3 (lightdock_<side>.nm.npy, C order)
};

struct ContactsDevice {
    int n_atoms = 0, n_rec_res = 0, n_lig_res = 0, n_lig_grp = 0;  // groups: kResGroup consecutive ligand residues
    int boxes_in_lds = 0;
    const uint32_t *res_start = nullptr;  // n_rec_res + n_lig_res + 1 complex atom indices, receptor residues first
    const uint32_t *res_of_atom = nullptr;  // n_atoms residue indices, the ligand's after the receptor's
    __host__ __device__ int n_boxes() const { return n_rec_res + n_lig_res + n_lig_grp; }
    size_t box_bytes() const { return (size_t)n_boxes() * 6 * sizeof(int); }
};

// Every launch reads `m` as ComplexDevice says and pose rows of 7 + m.anm_rec + m.anm_lig doubles, `stride` doubles apart.

// poses: n rows; out: n x (m.n_rec + m.n_lig) x 3 doubles.
hipError_t launch_complex_pose_xyz(const ComplexDevice &m, const double *poses, size_t stride, size_t n, double *out,
                                   hipStream_t stream);
// poses: n_swarms x G rows; backbone: n_bb complex atom indices; ws: n_swarms x n_bb x 3 x G int32; overflow: one int.
hipError_t launch_complex_pose_thousandths(const ComplexDevice &m, const double *poses, size_t stride, int n_swarms, int G,
                                           const uint32_t *backbone, int n_bb, int32_t *ws, int *overflow, hipStream_t stream);
// One workgroup a swarm.  ws: as complex_pose_thousandths left it; scoring, cluster_of, representatives: n_swarms x G;
// n_clusters: n_swarms.
hipError_t launch_complex_bsas(const int32_t *ws, const double *scoring, int n_swarms, int G, int n_bb, double cutoff,
                               int32_t *cluster_of, int32_t *representatives, uint32_t *n_clusters, hipStream_t stream);
// `slots` workgroups.  poses: n rows; d: as ContactsDevice says; atoms_ws: slots x d.n_atoms int4; boxes_ws: slots x 6 x
// d.n_boxes() ints, not read with d.boxes_in_lds; rec_bits: n x ceil(d.n_rec_res / 32) words; lig_bits: n x
// ceil(d.n_lig_res / 32) words (both sides together at most kMaxContactWords a pose); overflow: one int.
hipError_t launch_complex_contacts(const ComplexDevice &m, const ContactsDevice &d, const double *poses, size_t stride, size_t n,
                                   uint32_t C2, size_t slots, int4 *atoms_ws, int *boxes_ws, uint32_t *rec_bits,
                                   uint32_t *lig_bits, int *overflow, hipStream_t stream);

}  // namespace ld
