// prepare.cpp -- host side of K5 (prepare.hpp): the argument checks, one call's device memory, the lattice's bounds, the
// mask's compaction in node order, the sampling loop.
#include "prepare.hpp"

#include <string>

#include "device_memory.hpp"
#include "kernels/swarm_shell.hpp"

namespace ld {

namespace {

thread_local double g_last_kernel_ms = 0.0;

constexpr unsigned kCentreStepsPerCheck = 64;   // launches between two reads of the stop word

// The stream and the two events of one call.
struct Timeline {
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    Timeline() {
        try {
            hip_check(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "hipStreamCreate");
            hip_check(hipEventCreate(&ev0), "hipEventCreate");
            hip_check(hipEventCreate(&ev1), "hipEventCreate");
        } catch (...) {
            release();
            throw;
        }
    }
    Timeline(const Timeline &) = delete;
    Timeline &operator=(const Timeline &) = delete;
    ~Timeline() { release(); }
    void release() {
        if (stream) (void)hipStreamSynchronize(stream);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (stream) (void)hipStreamDestroy(stream);
        stream = nullptr;
        ev0 = ev1 = nullptr;
    }
    void start() { hip_check(hipEventRecord(ev0, stream), "hipEventRecord"); }
    void stop() { hip_check(hipEventRecord(ev1, stream), "hipEventRecord"); }
    // after a synchronisation that follows stop()
    void report() {
        float ms = 0.f;
        hip_check(hipEventElapsedTime(&ms, ev0, ev1), "hipEventElapsedTime");
        g_last_kernel_ms = ms;
    }
};

void check_coordinates(const int32_t *xyz, size_t n, size_t stride, const char *what) {
    for (size_t i = 0; i < n; i++)
        for (int c = 0; c < 3; c++) {
            const int32_t v = xyz[i * stride + c];
            if (v > kSwarmMaxCoordinate || v < -kSwarmMaxCoordinate)
                throw Error(LD_ERR_INVALID, std::string(what) + " " + std::to_string(i) + " lies beyond +-2000 A");
        }
}

}  // namespace

double setup_last_kernel_ms() { return g_last_kernel_ms; }

uint64_t swarm_diameter2(const int32_t *xyz, size_t n) {
    if (!xyz) throw Error(LD_ERR_INVALID, "null argument");
    if (n < 1 || n > kSwarmMaxDiameterAtoms) throw Error(LD_ERR_INVALID, "1 .. 2^20 atoms");
    check_coordinates(xyz, n, 3, "atom");
    Timeline t;
    DeviceArena arena;
    int *d_xyz = arena.upload(std::vector<int>(xyz, xyz + 3 * n));
    unsigned long long *d_max = arena.upload(std::vector<unsigned long long>(1, 0ull));
    g_last_kernel_ms = 0.0;
    t.start();
    hip_check(launch_swarm_diameter2(d_xyz, n, d_max, t.stream), "swarm_diameter2 launch");
    t.stop();
    unsigned long long d2 = 0;
    hip_check(hipMemcpyAsync(&d2, d_max, sizeof d2, hipMemcpyDeviceToHost, t.stream), "hipMemcpy D2H");
    hip_check(hipStreamSynchronize(t.stream), "swarm_diameter2");
    t.report();
    return d2;
}

SwarmShell swarm_shell(const int32_t *atoms, const uint8_t *bead, size_t n, int32_t spacing) {
    if (!atoms) throw Error(LD_ERR_INVALID, "null argument");
    if (n < 1 || n > 0x7fffffffu / 4) throw Error(LD_ERR_INVALID, "no atoms, or too many");
    if (spacing < 1 || spacing > kSwarmMaxSpacing) throw Error(LD_ERR_INVALID, "spacing must be 0.001 .. 1000 A");
    check_coordinates(atoms, n, 4, "atom");
    std::vector<int> words(4 * n);
    int lo[3], hi[3], e_max = 0;
    for (size_t i = 0; i < n; i++) {
        const int32_t E = atoms[4 * i + 3];
        if (E < 1 || E > kSwarmMaxExtent) throw Error(LD_ERR_INVALID, "the extent of atom " + std::to_string(i) + " must be 0.001 .. 4000 A");
        e_max = E > e_max ? E : e_max;
        for (int c = 0; c < 3; c++) {
            const int32_t v = atoms[4 * i + c];
            words[4 * i + c] = v;
            lo[c] = (i == 0 || v < lo[c]) ? v : lo[c];
            hi[c] = (i == 0 || v > hi[c]) ? v : hi[c];
        }
        words[4 * i + 3] = (int)((uint32_t)E | ((bead && bead[i]) ? kSwarmBeadBit : 0u));
    }
    SwarmLattice g;
    g.h = spacing;
    unsigned long long nodes = 1;
    for (int c = 0; c < 3; c++) {
        swarm_lattice_axis(lo[c], hi[c], e_max, spacing, &g.lo[c], &g.n[c]);
        // an axis alone can pass 2^28 when the spacing is small: the running product stays below 2^57
        if ((unsigned long long)g.n[c] > kSwarmMaxNodes) nodes = kSwarmMaxNodes + 1;
        if (nodes <= kSwarmMaxNodes) nodes *= (unsigned long long)g.n[c];
    }
    if (nodes > kSwarmMaxNodes)
        throw Error(LD_ERR_INVALID, "the lattice has more than 2^28 nodes: raise the spacing (" + std::to_string(spacing) + " thousandths)");

    Timeline t;
    DeviceArena arena;
    int *d_atoms = arena.upload(words);
    const size_t n_words = swarm_mask_words(nodes);
    unsigned long long *d_mask = static_cast<unsigned long long *>(arena.alloc_bytes(n_words * sizeof(unsigned long long)));
    g_last_kernel_ms = 0.0;
    t.start();
    hip_check(launch_swarm_shell(d_atoms, n, g, nodes, d_mask, t.stream), "swarm_shell launch");
    t.stop();
    std::vector<unsigned long long> mask(n_words);
    hip_check(hipMemcpyAsync(mask.data(), d_mask, n_words * sizeof(unsigned long long), hipMemcpyDeviceToHost, t.stream), "hipMemcpy D2H");
    hip_check(hipStreamSynchronize(t.stream), "swarm_shell");
    t.report();

    size_t count = 0;
    for (unsigned long long w : mask) count += (size_t)__builtin_popcountll(w);
    if (count > kSwarmMaxCandidates)
        throw Error(LD_ERR_INVALID, std::to_string(count) + " candidates, more than 2^22: raise the spacing (" + std::to_string(spacing) + " thousandths)");
    SwarmShell out;
    out.nodes = nodes;
    out.candidates.reserve(3 * count);
    for (size_t w = 0; w < n_words; w++)
        for (unsigned long long bits = mask[w]; bits; bits &= bits - 1) {
            const unsigned long long node = (unsigned long long)w * 64 + (unsigned)__builtin_ctzll(bits);
            if (node >= nodes) throw Error(LD_ERR_INTERNAL, "the shell's mask marks a node past the lattice");
            int p[3];
            swarm_node(g, node, &p[0], &p[1], &p[2]);
            out.candidates.insert(out.candidates.end(), p, p + 3);
        }
    return out;
}

SwarmCentres swarm_centres(const int32_t *points, size_t n, size_t max_centres, int32_t cover) {
    if (!points && n) throw Error(LD_ERR_INVALID, "null argument");
    if (n > kSwarmMaxCandidates) throw Error(LD_ERR_INVALID, "more than 2^22 points");
    if (max_centres < 1) throw Error(LD_ERR_INVALID, "max_centres must be positive");
    if (cover < 0) throw Error(LD_ERR_INVALID, "cover must not be negative");
    check_coordinates(points, n, 3, "point");
    SwarmCentres out;
    if (n == 0) return out;
    const size_t most = max_centres < n ? max_centres : n;
    const int groups = swarm_centre_groups(n);
    const long long cover2 = (long long)cover * cover;

    Timeline t;
    DeviceArena arena;
    int *d_xyz = arena.upload(std::vector<int>(points, points + 3 * n));
    long long *d_gap = static_cast<long long *>(arena.alloc_bytes(n * sizeof(long long)));
    SwarmPick *d_pick[2];
    for (auto &p : d_pick) p = static_cast<SwarmPick *>(arena.alloc_bytes((size_t)groups * sizeof(SwarmPick)));
    unsigned *d_index = static_cast<unsigned *>(arena.alloc_bytes(most * sizeof(unsigned)));
    unsigned long long *d_gap2 = static_cast<unsigned long long *>(arena.alloc_bytes(most * sizeof(unsigned long long)));
    unsigned *d_state = arena.upload(std::vector<unsigned>(2, 0u));

    g_last_kernel_ms = 0.0;
    t.start();
    unsigned state[2] = {0u, 0u};
    for (size_t step = 0; step <= most && !state[1]; step++) {
        hip_check(launch_swarm_centres_step(d_xyz, n, d_gap, d_pick[(step + 1) & 1], d_pick[step & 1], groups, (unsigned)step,
                                            step == most, cover2, d_index, d_gap2, d_state, t.stream),
                  "swarm_centres_step launch");
        if (cover2 > 0 && (step + 1) % kCentreStepsPerCheck == 0) {   // has the cover rule ended it?
            hip_check(hipMemcpyAsync(state, d_state, sizeof state, hipMemcpyDeviceToHost, t.stream), "hipMemcpy D2H");
            hip_check(hipStreamSynchronize(t.stream), "swarm_centres_step");
        }
    }
    t.stop();
    hip_check(hipMemcpyAsync(state, d_state, sizeof state, hipMemcpyDeviceToHost, t.stream), "hipMemcpy D2H");
    hip_check(hipStreamSynchronize(t.stream), "swarm_centres_step");
    t.report();
    const size_t count = state[0];
    if (count > most) throw Error(LD_ERR_INTERNAL, "the sampling kernel reports more centres than were asked for");
    out.index.resize(count);
    out.gap2.resize(count);
    if (count) {
        hip_check(hipMemcpy(out.index.data(), d_index, count * sizeof(unsigned), hipMemcpyDeviceToHost), "hipMemcpy D2H");
        hip_check(hipMemcpy(out.gap2.data(), d_gap2, count * sizeof(unsigned long long), hipMemcpyDeviceToHost), "hipMemcpy D2H");
    }
    return out;
}

}  // namespace ld
