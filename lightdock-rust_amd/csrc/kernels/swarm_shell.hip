// swarm_shell.hip -- K5, the swarm centres of a run (kernels/swarm_shell.hpp; lightdock_hip.h, "Preparing a
// run"): three plain kernels, exact integers throughout.
//   swarm_diameter2      the largest squared distance between two of n points: a thread a point, the others through LDS,
//                        one atomic max of an unsigned 64-bit value a workgroup (a maximum has no order).
//   swarm_shell          the hot path, nodes x atoms: a thread a lattice node, the atoms through LDS in tiles, a wave's
//                        64 verdicts stored as ONE word (its ballot), so the candidates' number and order are the mask's
//                        and do not depend on how the launch was cut.
//   swarm_centres_step   one step of farthest-point sampling.  No grid-wide wait: each step is a launch, a workgroup writes
//                        its own pick, and the NEXT launch's workgroups each reduce those picks (256 at most) to the same
//                        centre.  Picks are compared by (value, lowest index), never by arrival.
#include "kernels/swarm_shell.hpp"

namespace ld {

namespace {

__global__ __launch_bounds__(kSwarmThreads) void swarm_diameter2(const int *__restrict__ xyz, unsigned n,
                                                                 unsigned long long *__restrict__ d2_max) {
    __shared__ int tile[kSwarmThreads][3];
    __shared__ unsigned long long best[kSwarmThreads];
    const unsigned t = threadIdx.x, i = blockIdx.x * kSwarmThreads + t;
    const bool own = i < n;
    const int x = own ? xyz[3 * (size_t)i] : 0, y = own ? xyz[3 * (size_t)i + 1] : 0, z = own ? xyz[3 * (size_t)i + 2] : 0;
    long long largest = 0;
    for (unsigned base = 0; base < n; base += kSwarmThreads) {
        const unsigned j = base + t;
        __syncthreads();
        if (j < n) {
            tile[t][0] = xyz[3 * (size_t)j];
            tile[t][1] = xyz[3 * (size_t)j + 1];
            tile[t][2] = xyz[3 * (size_t)j + 2];
        }
        __syncthreads();
        const unsigned count = n - base < (unsigned)kSwarmThreads ? n - base : (unsigned)kSwarmThreads;
        if (own)
            for (unsigned a = 0; a < count; a++) {
                const long long d2 = swarm_dist2(x - tile[a][0], y - tile[a][1], z - tile[a][2]);
                largest = d2 > largest ? d2 : largest;
            }
    }
    best[t] = (unsigned long long)largest;
    __syncthreads();
    for (unsigned s = kSwarmThreads / 2; s > 0; s >>= 1) {
        if (t < s && best[t + s] > best[t]) best[t] = best[t + s];
        __syncthreads();
    }
    if (t == 0) atomicMax(d2_max, best[0]);
}

__global__ __launch_bounds__(kSwarmThreads) void swarm_shell(const int4 *__restrict__ atoms, unsigned n_atoms, SwarmLattice g,
                                                             unsigned long long nodes, unsigned long long *__restrict__ mask) {
    __shared__ int4 tile[kSwarmThreads];
    const unsigned t = threadIdx.x;
    const unsigned long long node = (unsigned long long)blockIdx.x * kSwarmThreads + t;
    const bool real = node < nodes;
    int px = 0, py = 0, pz = 0;
    if (real) swarm_node(g, node, &px, &py, &pz);
    bool outside = real, near = false;
    for (unsigned base = 0; base < n_atoms; base += kSwarmThreads) {
        __syncthreads();
        if (base + t < n_atoms) tile[t] = atoms[base + t];
        __syncthreads();
        const unsigned count = n_atoms - base < (unsigned)kSwarmThreads ? n_atoms - base : (unsigned)kSwarmThreads;
        for (unsigned a = 0; a < count; a++) {
            const int4 c = tile[a];
            swarm_node_test(px, py, pz, c.x, c.y, c.z, (uint32_t)c.w, g.h, &outside, &near);
        }
    }
    // every lane of the wave is here: the loop's bounds are the launch's, no lane has left
    const unsigned long long word = __ballot(outside && near);
    if ((t & 63u) == 0) mask[node >> 6] = word;
}

// The best of the workgroup's (v, i) in every thread.
__device__ void swarm_block_best(long long &v, unsigned &i, long long *sv, unsigned *si) {
    const unsigned t = threadIdx.x;
    sv[t] = v;
    si[t] = i;
    __syncthreads();
    for (unsigned s = kSwarmThreads / 2; s > 0; s >>= 1) {
        if (t < s && swarm_better(sv[t + s], si[t + s], sv[t], si[t])) {
            sv[t] = sv[t + s];
            si[t] = si[t + s];
        }
        __syncthreads();
    }
    v = sv[0];
    i = si[0];
    __syncthreads();
}

__global__ __launch_bounds__(kSwarmThreads) void swarm_centres_step(const int *__restrict__ xyz, unsigned n, long long *__restrict__ gap,
                                                                    const SwarmPick *__restrict__ in, SwarmPick *__restrict__ out,
                                                                    unsigned step, int last, long long cover2,
                                                                    unsigned *__restrict__ index_out,
                                                                    unsigned long long *__restrict__ gap2_out,
                                                                    unsigned *__restrict__ state) {
    __shared__ long long sv[kSwarmThreads];
    __shared__ unsigned si[kSwarmThreads];
    const unsigned t = threadIdx.x, groups = gridDim.x;
    unsigned chosen = kSwarmNoIndex;
    int lx = 0, ly = 0, lz = 0;
    if (step > 0) {   // uniform over the launch
        long long v = t < groups ? in[t].value : kSwarmNone;
        unsigned i = t < groups ? in[t].index : kSwarmNoIndex;
        swarm_block_best(v, i, sv, si);
        const bool stopped = v < 0 || i >= n || (step >= 2 && cover2 > 0 && v <= cover2);   // the same in every workgroup
        if (blockIdx.x == 0 && t == 0) {
            if (stopped) {
                state[1] = 1u;
            } else {
                index_out[step - 1] = i;
                gap2_out[step - 1] = (unsigned long long)v;
                state[0] = step;
            }
        }
        if (stopped || last) {
            if (t == 0) {
                SwarmPick none;
                none.value = kSwarmNone;
                none.index = kSwarmNoIndex;
                none.pad = 0;
                out[blockIdx.x] = none;
            }
            return;
        }
        chosen = i;
        lx = xyz[3 * (size_t)i];
        ly = xyz[3 * (size_t)i + 1];
        lz = xyz[3 * (size_t)i + 2];
    }
    long long bv = kSwarmNone;
    unsigned bi = kSwarmNoIndex;
    for (unsigned idx = blockIdx.x * kSwarmThreads + t; idx < n; idx += groups * kSwarmThreads) {
        const int x = xyz[3 * (size_t)idx], y = xyz[3 * (size_t)idx + 1], z = xyz[3 * (size_t)idx + 2];
        long long value;
        if (step == 0) {
            gap[idx] = 0x7fffffffffffffffll;
            value = swarm_dist2(x, y, z);
        } else {
            value = gap[idx];
            if (idx == chosen) {
                value = kSwarmNone;
                gap[idx] = value;
            } else if (value >= 0) {
                const long long d2 = swarm_dist2(x - lx, y - ly, z - lz);
                if (d2 < value) {
                    value = d2;
                    gap[idx] = value;
                }
            }
        }
        if (value >= 0 && swarm_better(value, idx, bv, bi)) {
            bv = value;
            bi = idx;
        }
    }
    swarm_block_best(bv, bi, sv, si);
    if (t == 0) {
        SwarmPick pick;
        pick.value = bv;
        pick.index = bi;
        pick.pad = 0;
        out[blockIdx.x] = pick;
    }
}

}  // namespace

hipError_t launch_swarm_diameter2(const int *xyz, size_t n, unsigned long long *d2_max, hipStream_t stream) {
    if (n < 1 || n > kSwarmMaxDiameterAtoms) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((n + kSwarmThreads - 1) / kSwarmThreads);
    hipLaunchKernelGGL(swarm_diameter2, dim3(blocks), dim3(kSwarmThreads), 0, stream, xyz, (unsigned)n, d2_max);
    return hipGetLastError();
}

hipError_t launch_swarm_shell(const int *atoms, size_t n_atoms, const SwarmLattice &g, unsigned long long nodes,
                              unsigned long long *mask, hipStream_t stream) {
    if (n_atoms < 1 || n_atoms > 0xffffffffull || nodes < 1 || nodes > kSwarmMaxNodes || g.h < 1) return hipErrorInvalidValue;
    if ((unsigned long long)g.n[0] * (unsigned long long)g.n[1] * (unsigned long long)g.n[2] != nodes) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((nodes + kSwarmThreads - 1) / kSwarmThreads);
    hipLaunchKernelGGL(swarm_shell, dim3(blocks), dim3(kSwarmThreads), 0, stream, reinterpret_cast<const int4 *>(atoms),
                       (unsigned)n_atoms, g, nodes, mask);
    return hipGetLastError();
}

hipError_t launch_swarm_centres_step(const int *xyz, size_t n, long long *gap, const SwarmPick *in, SwarmPick *out, int groups,
                                     unsigned step, bool last, long long cover2, unsigned *index_out,
                                     unsigned long long *gap2_out, unsigned *state, hipStream_t stream) {
    if (n < 1 || n > kSwarmMaxCandidates || groups != swarm_centre_groups(n) || in == out || (step == 0 && last)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(swarm_centres_step, dim3((unsigned)groups), dim3(kSwarmThreads), 0, stream, xyz, (unsigned)n, gap, in, out, step,
                       last ? 1 : 0, cover2, index_out, gap2_out, state);
    return hipGetLastError();
}

}  // namespace ld
