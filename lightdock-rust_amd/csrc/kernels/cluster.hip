// cluster.hip -- K3: the analysis half of a LightDock run (gfx950).  Kernels and their launchers
// (kernels/cluster.hpp); the host side is complex.cpp.
//   complex_pose_xyz:          poses x atoms -> posed f64 coordinates (ld_complex_coordinates, ld_complex_write_pdb);
//   complex_pose_thousandths:  poses x CA / P atoms -> posed coordinates as the integer thousandths "%8.3f" prints
//                              (lgd_cluster_bsas.py clusters the PDB files it wrote, so it sees exactly those);
//   complex_bsas:              one workgroup per swarm: sort (scoring desc, glowworm asc) in LDS, then the greedy BSAS
//                              pass one representative at a time;
//   complex_contacts:          one workgroup a pose: which receptor and which ligand residues touch (ld_complex_contacts;
//                              what lgd_filter_restraints.py and lgd_filter_membrane.py ask of a model's PDB file).
// Posing and the thousandths: kernels/complex_rule.hpp; the RMSD test: kernels/complex_pose.hpp, shared with kernels/ranked.hip.  Workspace: the thousandths of a
// chunk of swarms, at most kClusterWorkspaceBytes (or one swarm's n_glowworms x n_backbone x 12 B if more; 1czy: 420 KB a
// swarm); ld_complex_coordinates poses in chunks of that bound.
#include "kernels/cluster.hpp"

#include "kernels/complex_pose.hpp"

#include <algorithm>
#include <climits>
#include <cmath>

namespace ld {

namespace {

constexpr int kEarlyExitAtoms = 32;  // the RMSD test is re-checked on the partial sum every this many atoms

__global__ void __launch_bounds__(kPoseThreads) complex_pose_xyz(ComplexDevice m, const double *poses, size_t stride,
                                                                 size_t n, uint32_t n_atoms, double *out) {
    const size_t total = n * n_atoms;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t i = t / n_atoms;
        const uint32_t a = (uint32_t)(t - i * n_atoms);
        const P3 p = pose_atom(m, poses + i * stride, a);
        out[3 * t] = p.x;
        out[3 * t + 1] = p.y;
        out[3 * t + 2] = p.z;
    }
}

// ws[((s * n_bb + b) * 3 + c) * G + g]: glowworm-fastest, so that the lanes of complex_bsas read one swarm's
// row of a coordinate together.  *overflow is set when a thousandth does not fit an int32 (|x| > 2.1e6 A).
__global__ void __launch_bounds__(kPoseThreads) complex_pose_thousandths(ComplexDevice m, const double *poses, size_t stride,
                                                                         int n_swarms, int G, const uint32_t *backbone,
                                                                         int n_bb, int32_t *ws, int *overflow) {
    const size_t total = (size_t)n_swarms * n_bb * G;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int g = (int)(t % G);
        const size_t sb = t / G;  // s * n_bb + b
        const int b = (int)(sb % n_bb);
        const size_t s = sb / n_bb;
        int v[3];
        if (!posed_thousandths(m, poses + (s * G + g) * stride, backbone[b], INT_MAX, v)) *overflow = 1;
        for (int k = 0; k < 3; k++) ws[(sb * 3 + k) * G + g] = v[k];
    }
}

__global__ void __launch_bounds__(kBsasThreads) complex_bsas(const int32_t *ws, const double *scoring, int G, int n_bb,
                                                             double cutoff, int32_t *cluster_of, int32_t *representatives,
                                                             uint32_t *n_clusters) {
    __shared__ double s_key[kMaxGlowworms];  // scoring; after the sort: the state words (int32)
    __shared__ int s_order[kMaxGlowworms];   // sorted position -> glowworm
    __shared__ int s_next;
    const int s = blockIdx.x;
    const int tid = threadIdx.x;
    int P = 1;
    while (P < G) P <<= 1;
    for (int i = tid; i < P; i += kBsasThreads) {
        s_key[i] = i < G ? scoring[(size_t)s * G + i] : -INFINITY;  // scores are finite: padding sorts last
        s_order[i] = i;
    }
    __syncthreads();
    // bitonic sort into (score desc, glowworm asc): Python's stable sort of lgd_cluster_bsas.py
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += kBsasThreads) {
                const int l = i ^ j;
                if (l > i) {
                    const double ki = s_key[i], kl = s_key[l];
                    const int oi = s_order[i], ol = s_order[l];
                    const bool l_first = kl > ki || (kl == ki && ol < oi);
                    const bool i_first = ki > kl || (ki == kl && oi < ol);
                    if ((i & k) == 0 ? l_first : i_first) {
                        s_key[i] = kl;
                        s_key[l] = ki;
                        s_order[i] = ol;
                        s_order[l] = oi;
                    }
                }
            }
            __syncthreads();
        }
    }
    int *state = reinterpret_cast<int *>(s_key);  // cluster of each sorted position, -1 while unresolved
    for (int i = tid; i < G; i += kBsasThreads) state[i] = -1;
    __syncthreads();

    const int32_t *sw = ws + (size_t)s * n_bb * 3 * G;
    const double n_atoms = (double)n_bb;
    int rep = 0, cid = 0;
    while (rep < G) {
        const int r = s_order[rep];
        if (tid == 0) {
            state[rep] = cid;
            representatives[(size_t)s * G + cid] = r;
        }
        // every unresolved later glowworm against the newest representative
        for (int j = rep + 1 + tid; j < G; j += kBsasThreads) {
            if (state[j] != -1) continue;
            const int g = s_order[j];
            double S = 0.0;
            bool ok = true;
            for (int b0 = 0; b0 < n_bb && ok; b0 += kEarlyExitAtoms) {
                const int b1 = min(n_bb, b0 + kEarlyExitAtoms);
                for (int b = b0; b < b1; b++) {
                    const int32_t *row = sw + (size_t)b * 3 * G;
                    const double dx = (double)row[g] - (double)row[r];
                    const double dy = (double)row[G + g] - (double)row[G + r];
                    const double dz = (double)row[2 * G + g] - (double)row[2 * G + r];
                    S += dx * dx;
                    S += dy * dy;
                    S += dz * dz;
                }
                ok = within_cutoff(S, n_atoms, cutoff);  // a partial sum that fails, fails
            }
            if (ok) state[j] = cid;
        }
        __syncthreads();
        // the next representative: the first position after `rep` still unresolved (wave 0, 64 at a time;
        // the scans of all rounds together visit each position once)
        if (tid < 64) {
            int next = G;
            for (int base = rep + 1; base < G; base += 64) {
                const int p = base + tid;
                const unsigned long long open = __ballot(p < G && state[p] == -1);
                if (open) {
                    next = base + __ffsll(open) - 1;
                    break;
                }
            }
            if (tid == 0) s_next = next;
        }
        __syncthreads();
        rep = s_next;
        cid++;
        __syncthreads();
    }
    for (int j = tid; j < G; j += kBsasThreads) cluster_of[(size_t)s * G + s_order[j]] = state[j];
    for (int c = cid + tid; c < G; c += kBsasThreads) representatives[(size_t)s * G + c] = -1;
    if (tid == 0) n_clusters[s] = (uint32_t)cid;
}

unsigned grid_for(size_t total) {
    const size_t blocks = (total + kPoseThreads - 1) / kPoseThreads;
    return (unsigned)std::max<size_t>(1, std::min<size_t>(blocks, 8192));
}

// --- contacts: which receptor and which ligand residues of a pose touch (lightdock_hip.h, "Interface contacts") -------
// One kernel, one workgroup a pose at a time (a launch has at most kContactSlots workgroups, each with a workspace slot it
// reuses for pose blockIdx, blockIdx + gridDim, ...), all on the integer thousandths:
//   1. every atom is posed once and kept as int4 (x, y, z, 0) in the slot (global memory, read back through L2); the same
//      pass folds it into the int32 min / max box of its residue with atomicMin / atomicMax;
//   2. the boxes of every group of kResGroup consecutive LIGAND residues from those of its residues.  Boxes are in LDS
//      when they fit kMaxBoxLdsBytes, else in the slot (one generic pointer serves both);
//   3. the receptor residues, dealt to the waves round robin, are culled against the whole ligand's box (a lane each); a
//      surviving receptor residue against the ligand groups (a lane each), against the residues of a surviving group,
//      and a surviving residue pair is walked 8 x 8 atoms at a time, stopping at the first contact.  (Groups of
//      consecutive RECEPTOR residues cull nothing on 1k4c: its membrane beads follow each other in the file, not in space.)
//   4. bits are ORed in LDS and every output word is stored once.
// Every coordinate is within +-kComplexCoordBound (the call fails otherwise), so the difference of any two fits an int32.

// The boxes and their exact distance test: kernels/complex_pose.hpp, shared with kernels/fcc.hip.

// 8 waves a SIMD: four workgroups a CU hide the latency of the dependent loads
__global__ void __launch_bounds__(kContactThreads, 8) complex_contacts(ComplexDevice m, ContactsDevice d, const double *poses,
                                                                    size_t stride, size_t n, uint32_t C2, int4 *atoms_ws,
                                                                    int *boxes_ws, uint32_t *rec_bits, uint32_t *lig_bits,
                                                                    int *overflow) {
    extern __shared__ uint32_t s_bits[];  // receptor words, ligand words, then the boxes if they fit
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rw = (d.n_rec_res + 31) >> 5, lw = (d.n_lig_res + 31) >> 5;
    const int n_res = d.n_rec_res + d.n_lig_res, n_boxes = n_res + d.n_lig_grp;
    int4 *A = atoms_ws + (size_t)blockIdx.x * d.n_atoms;
    int *box = d.boxes_in_lds ? reinterpret_cast<int *>(s_bits + rw + lw) : boxes_ws + (size_t)blockIdx.x * 6 * n_boxes;
    const uint32_t *lig_start = d.res_start + d.n_rec_res;
    const int lig_grp = n_res;  // first group box
    const int lig_res = d.n_rec_res;

    for (size_t pose = blockIdx.x; pose < n; pose += gridDim.x) {
        const double *row = poses + pose * stride;
        for (int i = tid; i < rw + lw; i += kContactThreads) s_bits[i] = 0;
        for (int r = tid; r < n_res; r += kContactThreads)
            store_box(box, n_boxes, r, Box{{INT_MAX, INT_MAX, INT_MAX}, {INT_MIN, INT_MIN, INT_MIN}});
        __syncthreads();
        // every atom is posed once; its residue's box falls out of the same pass (min / max are order-free)
#pragma unroll 1
        for (int a = tid; a < d.n_atoms; a += kContactThreads) {
            int v[3];
            if (!posed_thousandths(m, row, (uint32_t)a, kComplexCoordBound, v)) *overflow = 1;
            const int r = (int)d.res_of_atom[a];
            for (int k = 0; k < 3; k++) {
                atomicMin(&box[k * n_boxes + r], v[k]);
                atomicMax(&box[(3 + k) * n_boxes + r], v[k]);
            }
            A[a] = make_int4(v[0], v[1], v[2], 0);
        }
        __syncthreads();
#pragma unroll 1
        for (int g = tid; g < d.n_lig_grp; g += kContactThreads) {
            const int r0 = lig_res + g * kResGroup, r1 = min(r0 + kResGroup, n_res);
            Box b = load_box(box, n_boxes, r0);
#pragma unroll 1
            for (int r = r0 + 1; r < r1; r++) {
                const Box o = load_box(box, n_boxes, r);
                for (int k = 0; k < 3; k++) b.lo[k] = min(b.lo[k], o.lo[k]), b.hi[k] = max(b.hi[k], o.hi[k]);
            }
            store_box(box, n_boxes, lig_grp + g, b);
        }
        __syncthreads();

        // all control flow below is uniform over the wave: the masks come from ballots
        // the whole ligand's box, every wave for itself: lanes over the groups, then a butterfly
        Box whole{{INT_MAX, INT_MAX, INT_MAX}, {INT_MIN, INT_MIN, INT_MIN}};
        for (int g = lane; g < d.n_lig_grp; g += 64) {
            const Box o = load_box(box, n_boxes, lig_grp + g);
            for (int k = 0; k < 3; k++) whole.lo[k] = min(whole.lo[k], o.lo[k]), whole.hi[k] = max(whole.hi[k], o.hi[k]);
        }
        for (int step = 1; step < 64; step <<= 1)
            for (int k = 0; k < 3; k++) {
                whole.lo[k] = min(whole.lo[k], __shfl_xor(whole.lo[k], step));
                whole.hi[k] = max(whole.hi[k], __shfl_xor(whole.hi[k], step));
            }
        // receptor residues are dealt to the waves round robin (neighbours in the file are neighbours in space, and
        // so are the residues of the interface): residue (64 i + lane) * waves + wave
        constexpr int kWaves = kContactThreads / 64;
        for (int base = 0; base * kWaves < d.n_rec_res; base += 64) {
            const int mine = (base + lane) * kWaves + wave;
            const Box mb = load_box(box, n_boxes, min(mine, d.n_rec_res - 1));
            unsigned long long residues = __builtin_amdgcn_ballot_w64(mine < d.n_rec_res && boxes_within(mb, whole, C2));
            while (residues) {
                const int rr = (base + __ffsll(residues) - 1) * kWaves + wave;
                residues &= residues - 1;
                const Box rb = load_box(box, n_boxes, rr);
                const uint32_t rbit = 1u << (rr & 31);
                const int a0 = (int)d.res_start[rr], a1 = (int)d.res_start[rr + 1];
                for (int lg0 = 0; lg0 < d.n_lig_grp; lg0 += 64) {
                    const int lg = lg0 + lane;
                    unsigned long long groups =
                        __builtin_amdgcn_ballot_w64(lg < d.n_lig_grp && boxes_within(rb, load_box(box, n_boxes, lig_grp + lg), C2));
                    while (groups) {
                        const int lgi = lg0 + __ffsll(groups) - 1;
                        groups &= groups - 1;
                        const int l = lgi * kResGroup + lane;  // the first kResGroup lanes: a ligand residue each
                        unsigned long long pairs = __builtin_amdgcn_ballot_w64(
                            lane < kResGroup && l < d.n_lig_res && boxes_within(rb, load_box(box, n_boxes, lig_res + l), C2));
                        while (pairs) {
                            const int ll = lgi * kResGroup + __ffsll(pairs) - 1;
                            pairs &= pairs - 1;
                            const uint32_t lbit = 1u << (ll & 31);
                            // the result is an OR: a pair whose two bits are set has nothing to add (a stale read of
                            // another wave's bit only costs the walk)
                            const uint32_t have_r = __builtin_amdgcn_readfirstlane(s_bits[rr >> 5]);
                            const uint32_t have_l = __builtin_amdgcn_readfirstlane(s_bits[rw + (ll >> 5)]);
                            if ((have_r & rbit) && (have_l & lbit)) continue;
                            const int b0 = (int)lig_start[ll], b1 = (int)lig_start[ll + 1];
                            bool hit = false;
                            for (int ta = a0; ta < a1 && !hit; ta += 8)
                                for (int tb = b0; tb < b1 && !hit; tb += 8) {
                                    const int a = ta + (lane >> 3), b = tb + (lane & 7);
                                    hit = __builtin_amdgcn_ballot_w64(a < a1 && b < b1 && in_contact(A[a], A[b], C2)) != 0;
                                }
                            if (hit && lane == 0) {
                                if (!(have_r & rbit)) atomicOr(&s_bits[rr >> 5], rbit);
                                if (!(have_l & lbit)) atomicOr(&s_bits[rw + (ll >> 5)], lbit);
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < rw; i += kContactThreads) rec_bits[pose * rw + i] = s_bits[i];
        for (int i = tid; i < lw; i += kContactThreads) lig_bits[pose * lw + i] = s_bits[rw + i];
        __syncthreads();  // the slot and the words are reused by the next pose
    }
}

}  // namespace

hipError_t launch_complex_pose_xyz(const ComplexDevice &m, const double *poses, size_t stride, size_t n, double *out,
                                   hipStream_t stream) {
    const uint32_t n_atoms = (uint32_t)(m.n_rec + m.n_lig);
    hipLaunchKernelGGL(complex_pose_xyz, dim3(grid_for(n * n_atoms)), dim3(kPoseThreads), 0, stream, m, poses, stride, n, n_atoms,
                       out);
    return hipGetLastError();
}

hipError_t launch_complex_pose_thousandths(const ComplexDevice &m, const double *poses, size_t stride, int n_swarms, int G,
                                           const uint32_t *backbone, int n_bb, int32_t *ws, int *overflow, hipStream_t stream) {
    hipLaunchKernelGGL(complex_pose_thousandths, dim3(grid_for((size_t)n_swarms * n_bb * G)), dim3(kPoseThreads), 0, stream, m,
                       poses, stride, n_swarms, G, backbone, n_bb, ws, overflow);
    return hipGetLastError();
}

hipError_t launch_complex_bsas(const int32_t *ws, const double *scoring, int n_swarms, int G, int n_bb, double cutoff,
                               int32_t *cluster_of, int32_t *representatives, uint32_t *n_clusters, hipStream_t stream) {
    hipLaunchKernelGGL(complex_bsas, dim3((unsigned)n_swarms), dim3(kBsasThreads), 0, stream, ws, scoring, G, n_bb, cutoff,
                       cluster_of, representatives, n_clusters);
    return hipGetLastError();
}

hipError_t launch_complex_contacts(const ComplexDevice &m, const ContactsDevice &d, const double *poses, size_t stride, size_t n,
                                   uint32_t C2, size_t slots, int4 *atoms_ws, int *boxes_ws, uint32_t *rec_bits,
                                   uint32_t *lig_bits, int *overflow, hipStream_t stream) {
    // the bit words of both sides, then the boxes if they fit
    const size_t words = ((size_t)d.n_rec_res + 31) / 32 + ((size_t)d.n_lig_res + 31) / 32;
    const size_t lds = words * sizeof(uint32_t) + (d.boxes_in_lds ? d.box_bytes() : 0);
    hipLaunchKernelGGL(complex_contacts, dim3((unsigned)slots), dim3(kContactThreads), lds, stream, m, d, poses, stride, n, C2,
                       atoms_ws, boxes_ws, rec_bits, lig_bits, overflow);
    return hipGetLastError();
}

}  // namespace ld
