// hip_stub_prepare.cpp -- TEST INFRASTRUCTURE for the sanitizer build of the host side (`make asan`, `make asan-prepare`): the
// launches of kernels/swarm_shell.hpp, beside tests/asan/hip_stub.cpp which stands in for the HIP runtime and every other
// kernel.  Device memory is host memory there, so ASan checks every extent below against what prepare.cpp allocated.  The
// launches do their kernels' work in plain C++ from the predicates both sides share (swarm_dist2, swarm_node_test,
// swarm_node, swarm_better), workgroup by workgroup as the kernels cut it, so the driver's answers are real ones.
#include <vector>

#include "kernels/swarm_shell.hpp"

namespace ld {

hipError_t launch_swarm_diameter2(const int *xyz, size_t n, unsigned long long *d2_max, hipStream_t) {
    if (n < 1 || n > kSwarmMaxDiameterAtoms) return hipErrorInvalidValue;
    unsigned long long best = *d2_max;
    for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j < n; j++) {
            const long long d2 = swarm_dist2(xyz[3 * i] - xyz[3 * j], xyz[3 * i + 1] - xyz[3 * j + 1], xyz[3 * i + 2] - xyz[3 * j + 2]);
            if ((unsigned long long)d2 > best) best = (unsigned long long)d2;
        }
    *d2_max = best;
    return hipSuccess;
}

hipError_t launch_swarm_shell(const int *atoms, size_t n_atoms, const SwarmLattice &g, unsigned long long nodes,
                              unsigned long long *mask, hipStream_t) {
    if (n_atoms < 1 || nodes < 1 || nodes > kSwarmMaxNodes || g.h < 1) return hipErrorInvalidValue;
    if ((unsigned long long)g.n[0] * (unsigned long long)g.n[1] * (unsigned long long)g.n[2] != nodes) return hipErrorInvalidValue;
    const size_t words = swarm_mask_words(nodes);
    for (size_t w = 0; w < words; w++) {   // a wave a word, the words past the lattice's end too
        unsigned long long word = 0;
        for (unsigned lane = 0; lane < 64; lane++) {
            const unsigned long long node = (unsigned long long)w * 64 + lane;
            if (node >= nodes) continue;
            int px, py, pz;
            swarm_node(g, node, &px, &py, &pz);
            bool outside = true, near = false;
            for (size_t a = 0; a < n_atoms; a++)
                swarm_node_test(px, py, pz, atoms[4 * a], atoms[4 * a + 1], atoms[4 * a + 2], (uint32_t)atoms[4 * a + 3], g.h, &outside, &near);
            if (outside && near) word |= 1ull << lane;
        }
        mask[w] = word;
    }
    return hipSuccess;
}

hipError_t launch_swarm_centres_step(const int *xyz, size_t n, long long *gap, const SwarmPick *in, SwarmPick *out, int groups,
                                     unsigned step, bool last, long long cover2, unsigned *index_out, unsigned long long *gap2_out,
                                     unsigned *state, hipStream_t) {
    if (n < 1 || n > kSwarmMaxCandidates || groups != swarm_centre_groups(n) || in == out || (step == 0 && last)) return hipErrorInvalidValue;
    const SwarmPick none = {kSwarmNone, kSwarmNoIndex, 0};
    unsigned chosen = kSwarmNoIndex;
    if (step > 0) {
        SwarmPick best = none;
        for (int b = 0; b < groups; b++)
            if (swarm_better(in[b].value, in[b].index, best.value, best.index)) best = in[b];
        const bool stopped = best.value < 0 || best.index >= n || (step >= 2 && cover2 > 0 && best.value <= cover2);
        if (stopped) {
            state[1] = 1u;
        } else {
            index_out[step - 1] = best.index;
            gap2_out[step - 1] = (unsigned long long)best.value;
            state[0] = step;
        }
        if (stopped || last) {
            for (int b = 0; b < groups; b++) out[b] = none;
            return hipSuccess;
        }
        chosen = best.index;
    }
    std::vector<SwarmPick> picks((size_t)groups, none);
    for (size_t idx = 0; idx < n; idx++) {
        SwarmPick &pick = picks[(idx / kSwarmThreads) % (size_t)groups];   // the workgroup of the kernel's strided loop
        long long value;
        if (step == 0) {
            gap[idx] = 0x7fffffffffffffffll;
            value = swarm_dist2(xyz[3 * idx], xyz[3 * idx + 1], xyz[3 * idx + 2]);
        } else {
            value = gap[idx];
            if (idx == chosen) {
                value = gap[idx] = kSwarmNone;
            } else if (value >= 0) {
                const long long d2 = swarm_dist2(xyz[3 * idx] - xyz[3 * (size_t)chosen], xyz[3 * idx + 1] - xyz[3 * (size_t)chosen + 1],
                                                 xyz[3 * idx + 2] - xyz[3 * (size_t)chosen + 2]);
                if (d2 < value) value = gap[idx] = d2;
            }
        }
        if (value >= 0 && swarm_better(value, (unsigned)idx, pick.value, pick.index)) {
            pick.value = value;
            pick.index = (unsigned)idx;
        }
    }
    for (int b = 0; b < groups; b++) out[b] = picks[(size_t)b];
    return hipSuccess;
}

}  // namespace ld
