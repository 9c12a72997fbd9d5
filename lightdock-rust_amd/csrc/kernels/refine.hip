// refine.hip -- the kernels of the local refinement (kernels/refine.hpp; include/lightdock_hip.h "Local refinement").
// Plain HIP for gfx950, no atomics: a pose's state has one writer, the wave that owns the pose in refine_select.
#include <hip/hip_runtime.h>

#include <climits>
#include <limits>

#include "refine.hpp"

namespace ld {

namespace {

__global__ __launch_bounds__(kRefineThreads) void refine_begin(const RefineLaunch L, const double *__restrict__ start_energy, const double trans_step,
                                                               const double rot_cos, const double rot_sin, const double nm_step) {
    const size_t p = (size_t)blockIdx.x * kRefineThreads + threadIdx.x;
    if (p >= L.n_poses) return;
    const RefineState &S = L.state;
    S.energy[p] = start_energy[p];
    S.trans_step[p] = trans_step;
    S.rot_cos[p] = rot_cos;
    S.rot_sin[p] = rot_sin;
    S.nm_step[p] = nm_step;
    S.halvings[p] = 0;
    S.accepted[p] = 0;
    S.evaluations[p] = 1;
    S.frozen[p] = 0;
}

// A workgroup per pose.  The pose goes through LDS; the K x pose_len elements of its trial rows are written in row order,
// so a wave's stores are contiguous wherever trial_stride == pose_len.
__global__ __launch_bounds__(kRefineThreads) void refine_trials(const RefineLaunch L, double *__restrict__ trials, const size_t trial_stride,
                                                                uint8_t *__restrict__ active) {
    __shared__ double row[kRefineMaxPoseLen];
    const size_t p = blockIdx.x;   // (the grid is n_poses workgroups)
    const int K = refine_trial_count(L.pose_len);
    const bool frozen = L.state.frozen[p] != 0;   // the same for the whole workgroup
    for (int j = threadIdx.x; j < K; j += kRefineThreads) active[p * (size_t)K + j] = frozen ? 0 : 1;
    if (frozen) return;
    for (int e = threadIdx.x; e < L.pose_len; e += kRefineThreads) row[e] = L.poses[p * L.stride + e];
    __syncthreads();
    const double dt = L.state.trans_step[p], c = L.state.rot_cos[p], s = L.state.rot_sin[p], dn = L.state.nm_step[p];
    double *out = trials + p * (size_t)K * trial_stride;
    const int elements = K * L.pose_len;
    for (int i = threadIdx.x; i < elements; i += kRefineThreads) {
        const int j = i / L.pose_len, e = i - j * L.pose_len;
        out[(size_t)j * trial_stride + e] = refine_trial_value(row, j, e, dt, c, s, dn);
    }
}

// A wave per pose: lanes stride over j, then a butterfly over (e, j) leaves the first maximum in every lane; lane 0 decides.
__global__ __launch_bounds__(kRefineThreads) void refine_select(const RefineLaunch L, const double *__restrict__ energies, const uint32_t max_halvings,
                                                                int16_t *__restrict__ history, const size_t history_stride) {
    const int lane = threadIdx.x & 63;
    const size_t p = (size_t)blockIdx.x * (kRefineThreads / 64) + (threadIdx.x >> 6);   // the same for the whole wave
    if (p >= L.n_poses) return;
    if (L.state.frozen[p]) {   // its energy row is whatever the scorer left there: not read
        if (lane == 0) history[p * history_stride] = kRefineNotEvaluated;
        return;
    }
    const int K = refine_trial_count(L.pose_len);
    const double *e_row = energies + p * (size_t)K;
    double e_best = -std::numeric_limits<double>::infinity();
    int j_best = INT_MAX;   // a lane without a trial loses to every trial
    for (int j = lane; j < K; j += 64) {
        double e = e_row[j];
        if (e != e) e = -std::numeric_limits<double>::infinity();   // NaN
        if (refine_better(e, j, e_best, j_best)) e_best = e, j_best = j;
    }
    for (int mask = 32; mask >= 1; mask >>= 1) {
        const double e_other = __shfl_xor(e_best, mask, 64);
        const int j_other = __shfl_xor(j_best, mask, 64);
        if (refine_better(e_other, j_other, e_best, j_best)) e_best = e_other, j_best = j_other;
    }
    if (lane == 0) history[p * history_stride] = refine_decide(L, p, e_best, j_best, max_halvings);
}

}  // namespace

hipError_t launch_refine_begin(const RefineLaunch &L, const double *start_energy, double trans_step, double rot_cos, double rot_sin,
                               double nm_step, hipStream_t stream) {
    if (L.n_poses == 0) return hipSuccess;
    const dim3 grid((unsigned)((L.n_poses + kRefineThreads - 1) / kRefineThreads));
    hipLaunchKernelGGL(refine_begin, grid, dim3(kRefineThreads), 0, stream, L, start_energy, trans_step, rot_cos, rot_sin, nm_step);
    return hipGetLastError();
}

hipError_t launch_refine_trials(const RefineLaunch &L, double *trials, size_t trial_stride, uint8_t *active, hipStream_t stream) {
    if (L.n_poses == 0) return hipSuccess;
    if (L.pose_len < 7 || L.pose_len > kRefineMaxPoseLen || L.stride < (size_t)L.pose_len || trial_stride < (size_t)L.pose_len ||
        L.n_poses > (size_t)INT_MAX)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(refine_trials, dim3((unsigned)L.n_poses), dim3(kRefineThreads), 0, stream, L, trials, trial_stride, active);
    return hipGetLastError();
}

hipError_t launch_refine_select(const RefineLaunch &L, const double *energies, uint32_t max_halvings, int16_t *history, size_t history_stride,
                                hipStream_t stream) {
    if (L.n_poses == 0) return hipSuccess;
    if (L.pose_len < 7 || L.pose_len > kRefineMaxPoseLen || L.stride < (size_t)L.pose_len || L.n_poses > (size_t)INT_MAX)
        return hipErrorInvalidValue;
    const size_t per_group = kRefineThreads / 64;
    hipLaunchKernelGGL(refine_select, dim3((unsigned)((L.n_poses + per_group - 1) / per_group)), dim3(kRefineThreads), 0, stream, L, energies,
                       max_halvings, history, history_stride);
    return hipGetLastError();
}

}  // namespace ld
