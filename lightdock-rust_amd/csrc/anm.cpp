// anm.cpp -- host side of K4 (anm.hpp): the argument checks, one call's device memory, the bounded sweep loop.
#include "anm.hpp"

#include <cmath>
#include <string>

#include "device_memory.hpp"
#include "kernels/anm.hpp"

namespace ld {

namespace {

thread_local double g_last_kernel_ms = 0.0;

std::string atom_name(const std::string &line) {
    std::string name = line.substr(12, 4);
    name.erase(name.find_last_not_of(' ') + 1);
    name.erase(0, name.find_first_not_of(' '));
    return name;
}

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
};

}  // namespace

std::vector<uint32_t> anm_node_atoms(const PdbFile &pdb) {
    const size_t n_res = pdb.res_id.size();
    std::vector<uint32_t> node(n_res);
    for (size_t r = 0; r < n_res; r++) {
        long ca = -1, c4 = -1;
        for (uint32_t a = pdb.res_start[r]; a < pdb.res_start[r + 1]; a++) {
            const std::string name = atom_name(pdb.lines[a]);
            if (ca < 0 && name == "CA") ca = a;
            if (c4 < 0 && name == "C4'") c4 = a;
        }
        if (ca < 0 && c4 < 0) throw Error(LD_ERR_INVALID, "residue " + pdb.res_id[r] + " has neither a CA nor a C4' atom: no node for it");
        node[r] = (uint32_t)(ca >= 0 ? ca : c4);
    }
    return node;
}

double anm_last_kernel_ms() { return g_last_kernel_ms; }

AnmResult anm_solve(const double *node_xyz, size_t m, size_t k, double cutoff, const uint32_t *node_of_atom, size_t n_atoms,
                    double rmsd) {
    if (!node_xyz) throw Error(LD_ERR_INVALID, "null argument");
    if (k == 0 || k > (size_t)kAnmMaxModes) throw Error(LD_ERR_INVALID, "n_modes must be 1 .. " + std::to_string(kAnmMaxModes));
    if (m > (size_t)kAnmMaxNodes) throw Error(LD_ERR_INVALID, "more than " + std::to_string(kAnmMaxNodes) + " nodes");
    if (3 * m < kAnmRigid + k)
        throw Error(LD_ERR_INVALID, std::to_string(m) + " nodes have " + std::to_string(3 * m) + " modes, six of them rigid: fewer than " +
                                        std::to_string(k) + " are left");
    if (!(cutoff > 0.0) || !std::isfinite(cutoff) || !std::isfinite(cutoff * cutoff)) throw Error(LD_ERR_INVALID, "cutoff must be positive and finite");
    if (!(rmsd >= 0.0) || !std::isfinite(rmsd)) throw Error(LD_ERR_INVALID, "rmsd must be finite and not negative");
    for (size_t i = 0; i < 3 * m; i++)
        if (!std::isfinite(node_xyz[i])) throw Error(LD_ERR_INVALID, "non-finite coordinate of node " + std::to_string(i / 3));
    if (!node_of_atom) n_atoms = m;
    if (n_atoms == 0) throw Error(LD_ERR_INVALID, "no atoms");
    std::vector<uint32_t> spread(n_atoms);
    for (size_t a = 0; a < n_atoms; a++) {
        spread[a] = node_of_atom ? node_of_atom[a] : (uint32_t)a;
        if (spread[a] >= m) throw Error(LD_ERR_INVALID, "atom " + std::to_string(a) + " names a node that does not exist");
    }

    const int nodes = (int)m, n = 3 * nodes, modes = (int)k;
    Timeline t;
    DeviceArena arena;
    const size_t cells = (size_t)n * n;
    double *d_xyz = arena.upload(std::vector<double>(node_xyz, node_xyz + 3 * m));
    uint32_t *d_spread = arena.upload(spread);
    double *d_A = static_cast<double *>(arena.alloc_bytes(cells * sizeof(double)));
    double *d_V = static_cast<double *>(arena.alloc_bytes(cells * sizeof(double)));
    double *d_sums = static_cast<double *>(arena.alloc_bytes((size_t)n * sizeof(double)));
    double *d_eig = static_cast<double *>(arena.alloc_bytes(k * sizeof(double)));
    double *d_scale = static_cast<double *>(arena.alloc_bytes(k * sizeof(double)));
    uint32_t *d_sel = static_cast<uint32_t *>(arena.alloc_bytes(k * sizeof(uint32_t)));
    unsigned long long *d_word = static_cast<unsigned long long *>(arena.alloc_bytes(sizeof(unsigned long long)));
    double *d_out = static_cast<double *>(arena.alloc_bytes(k * n_atoms * 3 * sizeof(double)));

    g_last_kernel_ms = 0.0;
    hip_check(hipEventRecord(t.ev0, t.stream), "hipEventRecord");
    hip_check(launch_anm_hessian(d_xyz, nodes, cutoff * cutoff, d_A, d_V, t.stream), "anm_hessian launch");
    hip_check(launch_anm_diagonal(nodes, d_A, t.stream), "anm_diagonal launch");
    // Gershgorin: no eigenvalue is above the largest absolute column sum.  A column whose norm is below n 2^-53 of that
    // bound is rounding noise of the large eigenvalues (the six rigid modes end there) and takes no further part: turned
    // against each other such columns never settle.  What the frozen columns cost a kept mode is their norm over its
    // eigenvalue, far inside the rounding of the solve itself as long as that eigenvalue is not floppy.
    hip_check(launch_anm_column_sums(d_A, n, 1, d_sums, t.stream), "anm_column_sums launch");
    std::vector<double> sums((size_t)n);
    hip_check(hipMemcpyAsync(sums.data(), d_sums, sums.size() * sizeof(double), hipMemcpyDeviceToHost, t.stream), "hipMemcpy D2H");
    hip_check(hipStreamSynchronize(t.stream), "anm_hessian");
    double bound = 0.0;
    for (double s : sums) bound = s > bound ? s : bound;
    const double null_norm = n * 0x1p-53 * bound, null2 = null_norm * null_norm;

    bool converged = false;
    for (int sweep = 0; sweep < kAnmMaxSweeps && !converged; sweep++) {
        hip_check(hipMemsetAsync(d_word, 0, sizeof(unsigned long long), t.stream), "hipMemset");
        for (int step = 0; step < anm_steps(n); step++)
            hip_check(launch_anm_jacobi_step(d_A, d_V, n, step, null2, d_word, t.stream), "anm_jacobi_step launch");
        unsigned long long word = 0;
        hip_check(hipMemcpyAsync(&word, d_word, sizeof word, hipMemcpyDeviceToHost, t.stream), "hipMemcpy D2H");
        hip_check(hipStreamSynchronize(t.stream), "anm_jacobi_step");
        converged = word == 0;   // no pair turned: every ratio is within kAnmConverged
    }
    if (!converged)
        throw Error(LD_ERR_INTERNAL, "the Jacobi sweeps did not converge within " + std::to_string(kAnmMaxSweeps) + " sweeps");

    AnmResult out;
    out.eigenvalues.resize(k);
    hip_check(launch_anm_column_sums(d_A, n, 0, d_sums, t.stream), "anm_column_sums launch");
    hip_check(launch_anm_select(d_sums, n, modes, d_sel, d_eig, t.stream), "anm_select launch");
    hip_check(hipMemcpyAsync(out.eigenvalues.data(), d_eig, k * sizeof(double), hipMemcpyDeviceToHost, t.stream), "hipMemcpy D2H");
    hip_check(hipStreamSynchronize(t.stream), "anm_select");
    if (!(out.eigenvalues[0] >= kAnmFloppy))
        throw Error(LD_ERR_INVALID, "the seventh eigenvalue is " + std::to_string(out.eigenvalues[0]) +
                                        ": the network is floppy, collinear or in pieces");
    const double *d_scale_arg = nullptr;
    if (rmsd > 0.0) {
        double inverse = 0.0;
        for (double e : out.eigenvalues) inverse += 1.0 / e;
        std::vector<double> scale(k);
        for (size_t r = 0; r < k; r++) scale[r] = rmsd * std::sqrt((double)n_atoms) / std::sqrt(inverse) / std::sqrt(out.eigenvalues[r]);
        hip_check(hipMemcpyAsync(d_scale, scale.data(), k * sizeof(double), hipMemcpyHostToDevice, t.stream), "hipMemcpy H2D");
        hip_check(hipStreamSynchronize(t.stream), "hipMemcpy H2D");   // scale leaves scope
        d_scale_arg = d_scale;
    }
    hip_check(launch_anm_extend(d_V, n, d_sel, modes, d_spread, n_atoms, d_scale_arg, d_out, t.stream), "anm_extend launch");
    hip_check(hipEventRecord(t.ev1, t.stream), "hipEventRecord");
    out.modes.resize(k * n_atoms * 3);
    hip_check(hipMemcpyAsync(out.modes.data(), d_out, out.modes.size() * sizeof(double), hipMemcpyDeviceToHost, t.stream), "hipMemcpy D2H");
    hip_check(hipStreamSynchronize(t.stream), "anm_extend");
    float ms = 0.f;
    hip_check(hipEventElapsedTime(&ms, t.ev0, t.ev1), "hipEventElapsedTime");
    g_last_kernel_ms = ms;
    return out;
}

}  // namespace ld
