// hip_stub_refine.cpp -- TEST INFRASTRUCTURE for the sanitizer build of the host side: the launches of kernels/refine.hpp,
// beside tests/asan/hip_stub.cpp which stands in for the HIP runtime and every other kernel.  Device memory is host memory
// there, so ASan checks every extent below against what refine.cpp allocated and carved.  These DO what their kernels do,
// in plain C++ over the rule of kernels/refine.hpp, with the extents as refine.hip indexes them.
#include <climits>
#include <limits>

#include "kernels/refine.hpp"

namespace ld {

hipError_t launch_refine_begin(const RefineLaunch &L, const double *start_energy, double trans_step, double rot_cos, double rot_sin,
                               double nm_step, hipStream_t) {
    const RefineState &S = L.state;
    for (size_t p = 0; p < L.n_poses; p++) {
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
    return hipSuccess;
}

hipError_t launch_refine_trials(const RefineLaunch &L, double *trials, size_t trial_stride, uint8_t *active, hipStream_t) {
    if (L.n_poses == 0) return hipSuccess;
    if (L.pose_len < 7 || L.pose_len > kRefineMaxPoseLen || L.stride < (size_t)L.pose_len || trial_stride < (size_t)L.pose_len)
        return hipErrorInvalidValue;
    const int K = refine_trial_count(L.pose_len);
    for (size_t p = 0; p < L.n_poses; p++) {
        const bool frozen = L.state.frozen[p] != 0;
        for (int j = 0; j < K; j++) active[p * (size_t)K + j] = frozen ? 0 : 1;
        if (frozen) continue;
        const double *row = L.poses + p * L.stride;
        for (int j = 0; j < K; j++)
            for (int e = 0; e < L.pose_len; e++)
                trials[(p * (size_t)K + j) * trial_stride + e] =
                    refine_trial_value(row, j, e, L.state.trans_step[p], L.state.rot_cos[p], L.state.rot_sin[p], L.state.nm_step[p]);
    }
    return hipSuccess;
}

hipError_t launch_refine_select(const RefineLaunch &L, const double *energies, uint32_t max_halvings, int16_t *history, size_t history_stride,
                                hipStream_t) {
    if (L.n_poses == 0) return hipSuccess;
    if (L.pose_len < 7 || L.pose_len > kRefineMaxPoseLen || L.stride < (size_t)L.pose_len) return hipErrorInvalidValue;
    const int K = refine_trial_count(L.pose_len);
    for (size_t p = 0; p < L.n_poses; p++) {
        if (L.state.frozen[p]) {
            history[p * history_stride] = kRefineNotEvaluated;
            continue;
        }
        double e_best = -std::numeric_limits<double>::infinity();
        int j_best = INT_MAX;
        for (int j = 0; j < K; j++) {
            double e = energies[p * (size_t)K + j];
            if (e != e) e = -std::numeric_limits<double>::infinity();
            if (refine_better(e, j, e_best, j_best)) e_best = e, j_best = j;
        }
        history[p * history_stride] = refine_decide(L, p, e_best, j_best, max_halvings);
    }
    return hipSuccess;
}

}  // namespace ld
