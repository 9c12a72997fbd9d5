// hip_stub_anm.cpp -- TEST INFRASTRUCTURE for the sanitizer build of the host side (`make asan`, `make asan-anm`): the
// launches of kernels/anm.hpp, beside tests/asan/hip_stub.cpp which stands in for the HIP runtime and every other kernel.
// Device memory is host memory there, so ASan checks every extent below against what anm.cpp allocated.  The launches do
// their kernels' work in plain C++ with the rules both sides share (anm_block, anm_pair, anm_rotation: host code too), the
// sums serial where the kernels' are trees: the same algorithm, not the same bits.  So the driver's answers are real ones.
#include <cmath>
#include <vector>

#include "kernels/anm.hpp"

namespace ld {

hipError_t launch_anm_hessian(const double *xyz, int m, double cutoff2, double *A, double *V, hipStream_t) {
    if (m < 1 || m > kAnmMaxNodes || !(cutoff2 > 0.0)) return hipErrorInvalidValue;
    const size_t n = 3 * (size_t)m;
    for (int i = 0; i < m; i++)
        for (int j = 0; j < m; j++) {
            double b[9] = {};
            if (i != j) anm_block(xyz + 3 * (size_t)i, xyz + 3 * (size_t)j, cutoff2, b);
            for (int a = 0; a < 3; a++)
                for (int c = 0; c < 3; c++) {
                    const size_t at = (3 * (size_t)j + c) * n + 3 * (size_t)i + a;
                    A[at] = b[3 * a + c];
                    V[at] = (i == j && a == c) ? 1.0 : 0.0;
                }
        }
    return hipSuccess;
}

hipError_t launch_anm_diagonal(int m, double *A, hipStream_t) {
    if (m < 1 || m > kAnmMaxNodes) return hipErrorInvalidValue;
    const size_t n = 3 * (size_t)m;
    for (int i = 0; i < m; i++) {
        double acc[9] = {};
        for (int j = 0; j < m; j++) {
            if (j == i) continue;
            for (int a = 0; a < 3; a++)
                for (int c = 0; c < 3; c++) acc[3 * a + c] += A[(3 * (size_t)j + c) * n + 3 * (size_t)i + a];
        }
        for (int a = 0; a < 3; a++)
            for (int c = 0; c < 3; c++) A[(3 * (size_t)i + c) * n + 3 * (size_t)i + a] = 0.0 - acc[3 * a + c];
    }
    return hipSuccess;
}

hipError_t launch_anm_column_sums(const double *A, int n, int absolute, double *out, hipStream_t) {
    if (n < 1) return hipErrorInvalidValue;
    for (int j = 0; j < n; j++) {
        const double *col = A + (size_t)j * n;
        double sum = 0.0;
        for (int i = 0; i < n; i++) sum += absolute ? std::fabs(col[i]) : col[i] * col[i];
        out[j] = sum;
    }
    return hipSuccess;
}

hipError_t launch_anm_jacobi_step(double *A, double *V, int n, int step, double null2, unsigned long long *max_word, hipStream_t) {
    if (n < 2 || step < 0 || step >= anm_steps(n) || !(null2 >= 0.0)) return hipErrorInvalidValue;
    std::vector<char> seen((size_t)n, 0);   // a step's pairs are disjoint: what lets the kernel run them side by side
    for (int k = 0; k < anm_pairs(n); k++) {
        int p, q;
        if (!anm_pair(n, step, k, &p, &q)) continue;
        if (p < 0 || p >= q || seen[p] || seen[q]) return hipErrorInvalidValue;
        seen[p] = seen[q] = 1;
        double *ap = A + (size_t)p * n, *aq = A + (size_t)q * n, *vp = V + (size_t)p * n, *vq = V + (size_t)q * n;
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
        for (int i = 0; i < n; i++) {
            alpha += ap[i] * ap[i];
            beta += aq[i] * aq[i];
            gamma += ap[i] * aq[i];
        }
        double c, s, ratio;
        if (!anm_rotation(alpha, beta, gamma, null2, &c, &s, &ratio)) continue;
        unsigned long long bits;
        static_assert(sizeof bits == sizeof ratio, "a double's bits");
        __builtin_memcpy(&bits, &ratio, sizeof bits);
        if (bits > *max_word) *max_word = bits;
        for (int i = 0; i < n; i++) {
            const double x = ap[i], y = aq[i], u = vp[i], w = vq[i];
            ap[i] = c * x - s * y;
            aq[i] = s * x + c * y;
            vp[i] = c * u - s * w;
            vq[i] = s * u + c * w;
        }
    }
    return hipSuccess;
}

hipError_t launch_anm_select(const double *sums, int n, int k, uint32_t *selected, double *eigenvalues, hipStream_t) {
    if (k < 1 || k > kAnmMaxModes || n < kAnmRigid + k) return hipErrorInvalidValue;
    for (int j = 0; j < n; j++) {
        int rank = 0;
        for (int i = 0; i < n; i++) rank += (sums[i] < sums[j] || (sums[i] == sums[j] && i < j)) ? 1 : 0;
        if (rank >= kAnmRigid && rank < kAnmRigid + k) {
            selected[rank - kAnmRigid] = (uint32_t)j;
            eigenvalues[rank - kAnmRigid] = std::sqrt(sums[j]);
        }
    }
    return hipSuccess;
}

hipError_t launch_anm_extend(const double *V, int n, const uint32_t *selected, int k, const uint32_t *node_of_atom, size_t n_atoms,
                             const double *scale, double *out, hipStream_t) {
    if (k < 1 || k > kAnmMaxModes || n < 3 || !n_atoms) return hipErrorInvalidValue;
    for (int r = 0; r < k; r++) {
        if (selected[r] >= (uint32_t)n) return hipErrorInvalidValue;
        const double *col = V + (size_t)selected[r] * n;
        int at = 0;
        for (int i = 1; i < n; i++)
            if (std::fabs(col[i]) > std::fabs(col[at])) at = i;
        const double sign = col[at] < 0.0 ? -1.0 : 1.0;
        double sum = 0.0;
        for (size_t a = 0; a < n_atoms; a++) {
            if (3 * (size_t)node_of_atom[a] + 2 >= (size_t)n) return hipErrorInvalidValue;
            const double *node = col + 3 * (size_t)node_of_atom[a];
            sum += node[0] * node[0] + node[1] * node[1] + node[2] * node[2];
        }
        const double norm = std::sqrt(sum);
        for (size_t a = 0; a < n_atoms; a++)
            for (int c = 0; c < 3; c++) {
                const double unit = sign * col[3 * (size_t)node_of_atom[a] + c] / norm;
                out[((size_t)r * n_atoms + a) * 3 + c] = scale ? unit * scale[r] : unit;
            }
    }
    return hipSuccess;
}

}  // namespace ld
