// swarm_shell.hpp -- launch interface of K5, the swarm centres of a run (kernels/swarm_shell.hip; DESIGN §5 K5;
// lightdock_hip.h, "Preparing a run"): what the host side (prepare.cpp) and the three kernels share, and the integer rule
// itself (a squared distance, the two shell tests, the lattice bounds, the order of two picks), which is host code too so
// that a CPU build restates it.  Every coordinate is an int32 in thousandths of an angstrom.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace ld {

constexpr int kSwarmThreads = 256;
constexpr int kSwarmMaxCoordinate = 2000000;          // |x| of an atom or a point, thousandths
constexpr int kSwarmMaxExtent = 4000000;              // E_b of an atom
constexpr int kSwarmMaxSpacing = 1000000;             // h
constexpr unsigned long long kSwarmMaxNodes = 1ull << 28;
constexpr size_t kSwarmMaxCandidates = (size_t)1 << 22;   // also the most points farthest-point sampling takes
constexpr size_t kSwarmMaxDiameterAtoms = (size_t)1 << 20;
constexpr int kSwarmMaxPartials = 256;                // workgroups of a sampling step: one workgroup reduces their picks
constexpr uint32_t kSwarmBeadBit = 0x80000000u;       // in the fourth word of a device atom: a bead attracts no node
constexpr long long kSwarmNone = -1;                  // the gap of a chosen point; the value of "no pick"
constexpr unsigned kSwarmNoIndex = 0xffffffffu;

// --- the rule, on integers ----------------------------------------------------------------------------------------------

// |d|^2.  |d_c| <= 10 000 000 (an atom within +-2e6, a node within +-2e6 +- E_max +- 2h): below 2^49.
__host__ __device__ inline long long swarm_dist2(int dx, int dy, int dz) {
    return (long long)dx * dx + ((long long)dy * dy + (long long)dz * dz);
}
// A node at squared distance d2 of an atom of extent E is not inside it: |p - c|^2 >= E^2.
__host__ __device__ inline bool swarm_outside(long long d2, int E) { return d2 >= (long long)E * E; }
// ... lies in the shell of width h about it: |p - c|^2 < (E + h)^2.
__host__ __device__ inline bool swarm_near(long long d2, int E, int h) {
    const long long reach = (long long)E + h;
    return d2 < reach * reach;
}
// The two tests of one device atom (x, y, z, E | bead bit) folded into a node's state.
__host__ __device__ inline void swarm_node_test(int px, int py, int pz, int cx, int cy, int cz, uint32_t word, int h, bool *outside,
                                                bool *near) {
    const int E = (int)(word & ~kSwarmBeadBit);
    const long long d2 = swarm_dist2(px - cx, py - cy, pz - cz);
    *outside = *outside && swarm_outside(d2, E);
    if (!(word & kSwarmBeadBit)) *near = *near || swarm_near(d2, E, h);
}

__host__ __device__ inline long long swarm_floor_div(long long a, long long b) { return a / b - ((a % b != 0 && (a < 0) != (b < 0)) ? 1 : 0); }
__host__ __device__ inline long long swarm_ceil_div(long long a, long long b) { return -swarm_floor_div(-a, b); }

// The lattice: node (i, j, k), 0 <= i < n[0] ..., lies at ((lo[0] + i) h, (lo[1] + j) h, (lo[2] + k) h); its number is
// (i n[1] + j) n[2] + k, which is the lexicographic order of its coordinates.
struct SwarmLattice {
    int lo[3];
    int n[3];
    int h;
};
// Per axis from floor((min c - E_max - h) / h) to ceil((max c + E_max + h) / h).
__host__ __device__ inline void swarm_lattice_axis(int min_c, int max_c, int e_max, int h, int *lo, int *count) {
    const long long first = swarm_floor_div((long long)min_c - e_max - h, h), last = swarm_ceil_div((long long)max_c + e_max + h, h);
    *lo = (int)first;
    *count = (int)(last - first + 1);
}
__host__ __device__ inline void swarm_node(const SwarmLattice &g, unsigned long long t, int *px, int *py, int *pz) {
    const int k = (int)(t % (unsigned)g.n[2]);
    const unsigned long long ij = t / (unsigned)g.n[2];
    const int j = (int)(ij % (unsigned)g.n[1]), i = (int)(ij / (unsigned)g.n[1]);
    *px = (g.lo[0] + i) * g.h;
    *py = (g.lo[1] + j) * g.h;
    *pz = (g.lo[2] + k) * g.h;
}

// Of two picks the one with the larger value wins, of equal values the lower index: no order of evaluation shows.
__host__ __device__ inline bool swarm_better(long long va, unsigned ia, long long vb, unsigned ib) {
    return va > vb || (va == vb && ia < ib);
}

struct SwarmPick {
    long long value;   // kSwarmNone: no point left, or sampling has stopped
    unsigned index;
    unsigned pad;
};

// Workgroups of one sampling step over n points: every point belongs to one, whatever their number.
inline int swarm_centre_groups(size_t n) {
    const size_t groups = (n + kSwarmThreads - 1) / kSwarmThreads;
    return (int)(groups < 1 ? 1 : groups > (size_t)kSwarmMaxPartials ? (size_t)kSwarmMaxPartials : groups);
}
// 64-bit words of the shell's mask: bit t % 64 of word t / 64 is node t; whole workgroups of kSwarmThreads nodes.
inline size_t swarm_mask_words(unsigned long long nodes) {
    return (size_t)((nodes + kSwarmThreads - 1) / kSwarmThreads) * (kSwarmThreads / 64);
}

// --- the launches -------------------------------------------------------------------------------------------------------

// *d2_max (ZEROED by the caller) = max over i, j of |x_i - x_j|^2 of n points (xyz: n x 3), by an atomic max of exact
// unsigned 64-bit values: a thread a point i, the points j through LDS.
hipError_t launch_swarm_diameter2(const int *xyz, size_t n, unsigned long long *d2_max, hipStream_t stream);
// mask: swarm_mask_words(nodes) words, every one written: a thread a node, a wave a word (its ballot), the atoms
// (n_atoms x 4 words: x, y, z, E | kSwarmBeadBit) through LDS.  Nodes past the lattice's end vote no.
hipError_t launch_swarm_shell(const int *atoms, size_t n_atoms, const SwarmLattice &g, unsigned long long nodes,
                              unsigned long long *mask, hipStream_t stream);
// One step of farthest-point sampling over n points (xyz: n x 3; gap: n), `groups` = swarm_centre_groups(n) workgroups.
//   step 0: gap = +inf; every workgroup's pick by |p|^2 goes to out[group].
//   step s > 0: every workgroup reduces in[0 .. groups) to the pick of centre s - 1.  No pick left, or s >= 2, cover2 > 0
//     and its value <= cover2: sampling has stopped (state[1] = 1) and out[group] says so to every later step.  Else
//     group 0 records index_out[s - 1], gap2_out[s - 1] and state[0] = s centres; then (unless `last`) the chosen point's
//     gap becomes kSwarmNone, every other gap the smaller of itself and the squared distance to it, and the workgroup's
//     pick by gap goes to out[group].
// in and out are different arrays of `groups` picks; state: two words, ZEROED before step 0.
hipError_t launch_swarm_centres_step(const int *xyz, size_t n, long long *gap, const SwarmPick *in, SwarmPick *out, int groups,
                                     unsigned step, bool last, long long cover2, unsigned *index_out,
                                     unsigned long long *gap2_out, unsigned *state, hipStream_t stream);

}  // namespace ld
