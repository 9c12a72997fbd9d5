// anm.hpp -- launch interface of K4, the normal modes of an anisotropic network model (kernels/anm.hip; DESIGN §5 K4;
// lightdock_hip.h, "Normal modes"): what the host side (anm.cpp) and the kernels share, and the small pieces of f64
// arithmetic that decide something (a node pair's block, a step's pairs, a rotation), which are host code too so that a CPU
// build runs the same rules.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace ld {

constexpr int kAnmThreads = 256;
constexpr int kAnmMaxNodes = 4096;
constexpr int kAnmMaxModes = 128;
constexpr int kAnmRigid = 6;        // the smallest eigenvalues that are rigid-body motions
constexpr int kAnmMaxSweeps = 40;
constexpr double kAnmConverged = 0x1p-50;   // |a_p . a_q| / (|a_p| |a_q|) at which a pair is left alone
constexpr double kAnmFloppy = 1e-6;         // a seventh eigenvalue below this is refused

// The 3 x 3 block of nodes i != j, row-major in b[9]: -(d d^T) / |d|^2 for 0 < |d|^2 <= cutoff2, else zero.  d = xj - xi;
// every product d_a d_b is the same for (j, i), so the matrix is symmetric to the bit.
__host__ __device__ inline void anm_block(const double *xi, const double *xj, double cutoff2, double b[9]) {
    const double d[3] = {xj[0] - xi[0], xj[1] - xi[1], xj[2] - xi[2]};
    const double d2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    const bool bound = d2 > 0.0 && d2 <= cutoff2;
    const double g = bound ? -1.0 / d2 : 0.0;
    for (int a = 0; a < 3; a++)
        for (int c = 0; c < 3; c++) b[3 * a + c] = bound ? (d[a] * d[c]) * g : 0.0;
}

// Round-robin schedule of n columns: N = n rounded up to even players, N - 1 steps a sweep, N / 2 disjoint pairs a step,
// every pair once a sweep.  Pair k of step s; false: the pair holds the player that does not exist (n odd), a bye.
__host__ __device__ inline int anm_steps(int n) { return ((n + 1) & ~1) - 1; }
__host__ __device__ inline int anm_pairs(int n) { return (n + 1) >> 1; }
__host__ __device__ inline bool anm_pair(int n, int step, int k, int *p, int *q) {
    const int ring = anm_steps(n);   // N - 1 players go round, player N - 1 stays
    int a, b;
    if (k == 0) {
        a = step;
        b = ring;
    } else {
        a = (step + k) % ring;
        b = (step - k + ring) % ring;
    }
    *p = a < b ? a : b;
    *q = a < b ? b : a;
    return *q < n;
}

// The rotation of one column pair from alpha = |a_p|^2, beta = |a_q|^2, gamma = a_p . a_q; null2: the square of the norm at
// which a column is rounding noise of the largest eigenvalue.  False: the pair is left alone.  *ratio = |gamma| /
// sqrt(alpha beta) of a pair that turns, what the sweep's convergence word collects.  a_p' = c a_p - s a_q, a_q' = s a_p + c a_q.
__host__ __device__ inline bool anm_rotation(double alpha, double beta, double gamma, double null2, double *c, double *s,
                                             double *ratio) {
    if (!(alpha > null2) || !(beta > null2)) return false;
    const double scale = sqrt(alpha) * sqrt(beta), g = fabs(gamma);
    if (!(g > kAnmConverged * scale)) return false;
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));   // an infinite zeta: t = 0
    *c = 1.0 / sqrt(1.0 + t * t);
    *s = *c * t;
    *ratio = g / scale;
    return true;
}

// The launches.  A and V: n x n doubles, column-major (column j at j * n), n = 3 m.

// A = the Hessian of m nodes (xyz: m x 3) without its diagonal blocks, V = I: a thread a node pair.
hipError_t launch_anm_hessian(const double *xyz, int m, double cutoff2, double *A, double *V, hipStream_t stream);
// The diagonal blocks: minus the sum of the row's other blocks, j ascending; a thread a node.
hipError_t launch_anm_diagonal(int m, double *A, hipStream_t stream);
// out[j] = sum_i |A_ij| (absolute != 0) or sum_i A_ij^2, a workgroup a column, a fixed-shape sum.
hipError_t launch_anm_column_sums(const double *A, int n, int absolute, double *out, hipStream_t stream);
// One step of a sweep: a workgroup a pair of the schedule.  max_word: the largest ratio of the turning pairs so far, as the
// bits of a non-negative double (their order is the integers' order), by atomic max.
hipError_t launch_anm_jacobi_step(double *A, double *V, int n, int step, double null2, unsigned long long *max_word,
                                  hipStream_t stream);
// sums: n column sums of squares.  The columns of rank kAnmRigid .. kAnmRigid + k - 1 in ascending order (ties: the lower
// column first): selected[r] = the column, eigenvalues[r] = sqrt(its sum).  n >= kAnmRigid + k.
hipError_t launch_anm_select(const double *sums, int n, int k, uint32_t *selected, double *eigenvalues, hipStream_t stream);
// A workgroup a mode: column selected[r] of V, its component of largest magnitude (the lowest index on a tie) made
// positive, spread over atoms (node_of_atom: n_atoms node indices), divided by its norm over all atoms x 3 and multiplied
// by scale[r] (scale NULL: 1).  out: k x n_atoms x 3.
hipError_t launch_anm_extend(const double *V, int n, const uint32_t *selected, int k, const uint32_t *node_of_atom,
                             size_t n_atoms, const double *scale, double *out, hipStream_t stream);

}  // namespace ld
