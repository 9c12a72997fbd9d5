// anm.hip -- K4: the normal modes of an anisotropic network model for gfx950 (launch interface and the shared rules:
// kernels/anm.hpp).
//
// The eigensolver is a one-sided (Hestenes) Jacobi iteration on the dense Hessian: A starts as H, V as I, every rotation is
// applied to the same two columns of both, so A = H V throughout; when the columns of A are orthogonal their norms are the
// eigenvalues and the columns of V the eigenvectors.  A step of the round-robin schedule touches every column at most once,
// so its pairs are independent: one launch a step, one workgroup a pair, no workgroup reads what another writes.  Nothing
// waits inside a launch; the host counts the sweeps.
//
// Every sum has a fixed shape (a thread's strided run, a shuffle tree over the wave, the four waves in order), so the same
// input gives the same bits.  The sweep's convergence word is an integer atomic max, which has no order to depend on.
#include "kernels/anm.hpp"

namespace ld {
namespace {

constexpr int kWaves = kAnmThreads / 64;

__device__ inline double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;   // lane 0 holds the sum
}

// The sums of up to three values over the workgroup, the same bits in every thread.  lds: 3 * kWaves doubles.
template <int K>
__device__ inline void block_sums(double (&v)[K], double *lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 0; k < K; k++) {
        const double w = wave_sum(v[k]);
        if (lane == 0) lds[k * kWaves + wave] = w;
    }
    __syncthreads();
    for (int k = 0; k < K; k++) {
        double total = lds[k * kWaves];
        for (int w = 1; w < kWaves; w++) total += lds[k * kWaves + w];
        v[k] = total;
    }
    __syncthreads();   // lds is free again
}

__global__ __launch_bounds__(kAnmThreads) void anm_hessian(const double *__restrict__ xyz, int m, double cutoff2,
                                                             double *__restrict__ A, double *__restrict__ V) {
    const int i = blockIdx.x * 64 + threadIdx.x;        // the rows: neighbouring lanes write neighbouring rows
    const int j = blockIdx.y * (kAnmThreads / 64) + threadIdx.y;
    if (i >= m || j >= m) return;
    const size_t n = 3 * (size_t)m;
    double b[9];
    if (i == j) {
        for (int e = 0; e < 9; e++) b[e] = 0.0;
    } else {
        anm_block(xyz + 3 * (size_t)i, xyz + 3 * (size_t)j, cutoff2, b);
    }
    for (int a = 0; a < 3; a++)
        for (int c = 0; c < 3; c++) {
            const size_t at = (3 * (size_t)j + c) * n + 3 * (size_t)i + a;
            A[at] = b[3 * a + c];
            V[at] = (i == j && a == c) ? 1.0 : 0.0;
        }
}

__global__ __launch_bounds__(kAnmThreads) void anm_diagonal(int m, double *__restrict__ A) {
    const int i = blockIdx.x * kAnmThreads + threadIdx.x;
    if (i >= m) return;
    const size_t n = 3 * (size_t)m;
    double acc[9] = {};
    for (int j = 0; j < m; j++) {
        if (j == i) continue;
        for (int a = 0; a < 3; a++)
            for (int c = 0; c < 3; c++) acc[3 * a + c] += A[(3 * (size_t)j + c) * n + 3 * (size_t)i + a];
    }
    for (int a = 0; a < 3; a++)
        for (int c = 0; c < 3; c++) A[(3 * (size_t)i + c) * n + 3 * (size_t)i + a] = 0.0 - acc[3 * a + c];
}

__global__ __launch_bounds__(kAnmThreads) void anm_column_sums(const double *__restrict__ A, int n, int absolute,
                                                                 double *__restrict__ out) {
    __shared__ double lds[kWaves];
    const double *col = A + (size_t)blockIdx.x * n;
    double v[1] = {0.0};
    for (int i = threadIdx.x; i < n; i += kAnmThreads) {
        const double x = col[i];
        v[0] += absolute ? fabs(x) : x * x;
    }
    block_sums(v, lds);
    if (threadIdx.x == 0) out[blockIdx.x] = v[0];
}

__global__ __launch_bounds__(kAnmThreads) void anm_jacobi_step(double *__restrict__ A, double *__restrict__ V, int n, int step,
                                                                 double null2, unsigned long long *max_word) {
    __shared__ double lds[3 * kWaves];
    int p, q;
    if (!anm_pair(n, step, (int)blockIdx.x, &p, &q)) return;   // the bye of an odd n
    double *ap = A + (size_t)p * n, *aq = A + (size_t)q * n;
    double v[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n; i += kAnmThreads) {
        const double x = ap[i], y = aq[i];
        v[0] += x * x;
        v[1] += y * y;
        v[2] += x * y;
    }
    block_sums(v, lds);
    double c, s, ratio;
    if (!anm_rotation(v[0], v[1], v[2], null2, &c, &s, &ratio)) return;   // the same decision in every thread
    if (threadIdx.x == 0) atomicMax(max_word, (unsigned long long)__double_as_longlong(ratio));
    double *vp = V + (size_t)p * n, *vq = V + (size_t)q * n;
    for (int i = threadIdx.x; i < n; i += kAnmThreads) {
        const double x = ap[i], y = aq[i];
        ap[i] = c * x - s * y;
        aq[i] = s * x + c * y;
        const double u = vp[i], w = vq[i];
        vp[i] = c * u - s * w;
        vq[i] = s * u + c * w;
    }
}

__global__ __launch_bounds__(kAnmThreads) void anm_select(const double *__restrict__ sums, int n, int k,
                                                            uint32_t *__restrict__ selected, double *__restrict__ eigenvalues) {
    const int j = blockIdx.x * kAnmThreads + threadIdx.x;
    if (j >= n) return;
    const double mine = sums[j];
    int rank = 0;
    for (int i = 0; i < n; i++) {
        const double other = sums[i];
        rank += (other < mine || (other == mine && i < j)) ? 1 : 0;
    }
    if (rank >= kAnmRigid && rank < kAnmRigid + k) {
        selected[rank - kAnmRigid] = (uint32_t)j;
        eigenvalues[rank - kAnmRigid] = sqrt(mine);
    }
}

__global__ __launch_bounds__(kAnmThreads) void anm_extend(const double *__restrict__ V, int n, const uint32_t *__restrict__ selected,
                                                            const uint32_t *__restrict__ node_of_atom, size_t n_atoms,
                                                            const double *__restrict__ scale, double *__restrict__ out) {
    __shared__ double lds[kWaves];
    __shared__ int lds_at[kWaves];
    const int r = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double *col = V + (size_t)selected[r] * n;
    // the component of largest magnitude, the lowest index on a tie
    double best = -1.0;
    int at = n;
    for (int i = threadIdx.x; i < n; i += kAnmThreads) {
        const double a = fabs(col[i]);
        if (a > best) {   // a thread's indices ascend: the first of equals stays
            best = a;
            at = i;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double b = __shfl_down(best, off, 64);
        const int bi = __shfl_down(at, off, 64);
        if (b > best || (b == best && bi < at)) {
            best = b;
            at = bi;
        }
    }
    if (lane == 0) {
        lds[wave] = best;
        lds_at[wave] = at;
    }
    __syncthreads();
    best = lds[0];
    at = lds_at[0];
    for (int w = 1; w < kWaves; w++)
        if (lds[w] > best || (lds[w] == best && lds_at[w] < at)) {
            best = lds[w];
            at = lds_at[w];
        }
    __syncthreads();
    const double sign = col[at] < 0.0 ? -1.0 : 1.0;
    // the norm over all atoms x 3
    double v[1] = {0.0};
    for (size_t a = threadIdx.x; a < n_atoms; a += kAnmThreads) {
        const double *node = col + 3 * (size_t)node_of_atom[a];
        v[0] += node[0] * node[0] + node[1] * node[1] + node[2] * node[2];
    }
    block_sums(v, lds);
    const double norm = sqrt(v[0]);
    double *mode = out + (size_t)r * n_atoms * 3;
    for (size_t a = threadIdx.x; a < n_atoms; a += kAnmThreads) {
        const double *node = col + 3 * (size_t)node_of_atom[a];
        for (int c = 0; c < 3; c++) {
            const double unit = sign * node[c] / norm;
            mode[3 * a + c] = scale ? unit * scale[r] : unit;
        }
    }
}

}  // namespace

hipError_t launch_anm_hessian(const double *xyz, int m, double cutoff2, double *A, double *V, hipStream_t stream) {
    const dim3 block(64, kAnmThreads / 64), grid((unsigned)((m + 63) / 64), (unsigned)((m + block.y - 1) / block.y));
    hipLaunchKernelGGL(anm_hessian, grid, block, 0, stream, xyz, m, cutoff2, A, V);
    return hipGetLastError();
}

hipError_t launch_anm_diagonal(int m, double *A, hipStream_t stream) {
    hipLaunchKernelGGL(anm_diagonal, dim3((unsigned)((m + kAnmThreads - 1) / kAnmThreads)), dim3(kAnmThreads), 0, stream, m, A);
    return hipGetLastError();
}

hipError_t launch_anm_column_sums(const double *A, int n, int absolute, double *out, hipStream_t stream) {
    hipLaunchKernelGGL(anm_column_sums, dim3((unsigned)n), dim3(kAnmThreads), 0, stream, A, n, absolute, out);
    return hipGetLastError();
}

hipError_t launch_anm_jacobi_step(double *A, double *V, int n, int step, double null2, unsigned long long *max_word,
                                  hipStream_t stream) {
    hipLaunchKernelGGL(anm_jacobi_step, dim3((unsigned)anm_pairs(n)), dim3(kAnmThreads), 0, stream, A, V, n, step, null2, max_word);
    return hipGetLastError();
}

hipError_t launch_anm_select(const double *sums, int n, int k, uint32_t *selected, double *eigenvalues, hipStream_t stream) {
    hipLaunchKernelGGL(anm_select, dim3((unsigned)((n + kAnmThreads - 1) / kAnmThreads)), dim3(kAnmThreads), 0, stream, sums, n, k,
                       selected, eigenvalues);
    return hipGetLastError();
}

hipError_t launch_anm_extend(const double *V, int n, const uint32_t *selected, int k, const uint32_t *node_of_atom, size_t n_atoms,
                             const double *scale, double *out, hipStream_t stream) {
    hipLaunchKernelGGL(anm_extend, dim3((unsigned)k), dim3(kAnmThreads), 0, stream, V, n, selected, node_of_atom, n_atoms, scale, out);
    return hipGetLastError();
}

}  // namespace ld
