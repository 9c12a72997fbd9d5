// assess.hip -- K3d: model quality against a reference complex (gfx950; lightdock_hip.h, "Model quality").
// Kernels and their launchers (kernels/assess.hpp); the host side is complex.cpp.
//   complex_assess_sums:   one workgroup a pose at a time (a launch has at most kAssessSlots workgroups, each with a
//                          workspace slot it reuses for pose blockIdx, blockIdx + gridDim, ...):
//     1. every USED atom (fit atoms and the matched atoms of residues of a native pair) is posed once, rounded to the
//        thousandths "%8.3f" prints and kept as int4 in the slot; the lane that posed a fit atom adds its terms to the
//        integer sums of its sets in registers (64-bit multiply-adds of 32-bit operands: every factor is below 2^21, every
//        sum below 2^64), a butterfly adds the lanes of a wave, and the waves meet in LDS with integer atomics;
//     2. the native pairs are dealt to the waves round robin; a pair is walked 8 x 8 atoms at a time with the 32-bit clamped
//        test of the contacts kernel, stopping at the first contact; a wave counts its pairs in a scalar;
//     3. the 40 words of the pose are stored once.
//   complex_assess_solve:  a thread a pose: the two eigenproblems and the ligand's trace in f64 (assess_solve_pose).
// Integer sums are order-free, so a pose's words, and with them its results, are the same bits whatever the batch, its
// place in it or the slot count.  No floating-point atomic anywhere.
#include "kernels/assess.hpp"

#include "kernels/complex_pose.hpp"

namespace ld {

namespace {

struct SetSums {
    long long w[kAssessSetWords];
};

__device__ __forceinline__ void clear(SetSums &s) {
#pragma unroll
    for (int k = 0; k < kAssessSetWords; k++) s.w[k] = 0;
}

// The terms of one atom; `on` = 0 leaves the sums as they are.
__device__ __forceinline__ void add_atom(SetSums &s, const int v[3], const int4 &ref, int on) {
    const int m[3] = {on ? v[0] : 0, on ? v[1] : 0, on ? v[2] : 0};
    const int r[3] = {ref.x, ref.y, ref.z};
    s.w[3] += (long long)m[0] * m[0] + (long long)m[1] * m[1] + (long long)m[2] * m[2];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        s.w[a] += m[a];
#pragma unroll
        for (int b = 0; b < 3; b++) s.w[4 + 3 * a + b] += (long long)m[a] * r[b];
    }
}

// The wave's total of every word, added to dst[0 .. 13) by lane 0.
__device__ __forceinline__ void flush(const SetSums &s, unsigned long long *dst, int lane) {
#pragma unroll
    for (int k = 0; k < kAssessSetWords; k++) {
        long long v = s.w[k];
#pragma unroll
        for (int step = 1; step < 64; step <<= 1) v += __shfl_xor(v, step);
        if (lane == 0 && v != 0) atomicAdd(dst + k, (unsigned long long)v);
    }
}

__global__ void __launch_bounds__(kAssessThreads, 4) complex_assess_sums(ComplexDevice m, AssessDevice d, const double *poses,
                                                                        size_t stride, size_t n, uint32_t C2, int4 *atoms_ws,
                                                                        long long *sums, int *overflow) {
    __shared__ unsigned long long s_words[kAssessWords];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int4 *A = atoms_ws + (size_t)blockIdx.x * d.n_used;

    for (size_t pose = blockIdx.x; pose < n; pose += gridDim.x) {
        const double *row = poses + pose * stride;
        if (tid < kAssessWords) s_words[tid] = 0;
        __syncthreads();
        SetSums side, both;  // the fit atoms of the side in hand; the interface fit atoms of both sides
        clear(side);
        clear(both);
#pragma unroll 1
        for (int half = 0; half < 2; half++) {
            const int u1 = half == 0 ? d.n_used_rec : d.n_used;
#pragma unroll 1
            for (int u = (half == 0 ? 0 : d.n_used_rec) + tid; u < u1; u += kAssessThreads) {
                int v[3];
                if (!posed_thousandths(m, row, d.used_atom[u], kAssessBound, v)) *overflow = 1;
                A[u] = make_int4(v[0], v[1], v[2], 0);
                const int4 ref = d.used_ref[u];
                add_atom(side, v, ref, ref.w & 1);
                add_atom(both, v, ref, (ref.w >> 1) & 1);
            }
            flush(side, s_words + (half == 0 ? kAssessRec : kAssessLig), lane);
            clear(side);
        }
        flush(both, s_words + kAssessInt, lane);
        __syncthreads();  // the slot's atoms are written

        // all control flow below is uniform over the wave
        constexpr int kWaves = kAssessThreads / 64;
        uint32_t kept = 0;
#pragma unroll 1
        for (int p = wave; p < d.n_native; p += kWaves) {
            const int4 pr = d.native[p];
            bool hit = false;
            for (int ta = pr.x; ta < pr.y && !hit; ta += 8)
                for (int tb = pr.z; tb < pr.w && !hit; tb += 8) {
                    const int a = ta + (lane >> 3), b = tb + (lane & 7);
                    hit = __builtin_amdgcn_ballot_w64(a < pr.y && b < pr.w && in_contact(A[a], A[b], C2)) != 0;
                }
            kept += hit ? 1u : 0u;
        }
        if (lane == 0 && kept) atomicAdd(&s_words[kAssessKept], (unsigned long long)kept);
        __syncthreads();
        if (tid < kAssessWords) sums[pose * kAssessWords + tid] = (long long)s_words[tid];
        __syncthreads();  // the slot and the words are reused by the next pose
    }
}

__global__ void __launch_bounds__(256) complex_assess_solve(AssessSolve k, const long long *sums, size_t n, uint32_t *kept,
                                                            double *lrmsd, double *irmsd) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    long long w[kAssessWords];
#pragma unroll
    for (int j = 0; j < kAssessWords; j++) w[j] = sums[i * kAssessWords + j];
    double l, r;
    assess_solve_pose(k, w, &l, &r);
    kept[i] = (uint32_t)w[kAssessKept];
    lrmsd[i] = l;
    irmsd[i] = r;
}

}  // namespace

hipError_t launch_complex_assess_sums(const ComplexDevice &m, const AssessDevice &d, const double *poses, size_t stride, size_t n,
                                      uint32_t C2, size_t slots, int4 *atoms_ws, long long *sums, int *overflow,
                                      hipStream_t stream) {
    hipLaunchKernelGGL(complex_assess_sums, dim3((unsigned)slots), dim3(kAssessThreads), 0, stream, m, d, poses, stride, n, C2,
                       atoms_ws, sums, overflow);
    return hipGetLastError();
}

hipError_t launch_complex_assess_solve(const AssessSolve &k, const long long *sums, size_t n, uint32_t *kept, double *lrmsd,
                                       double *irmsd, hipStream_t stream) {
    hipLaunchKernelGGL(complex_assess_solve, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, k, sums, n, kept, lrmsd, irmsd);
    return hipGetLastError();
}

}  // namespace ld
