// refine.hpp -- launch interface of the local refinement's kernels (kernels/refine.hip; include/lightdock_hip.h "Local
// refinement"): the state of a pose, the rule's arithmetic (host code too, so that a CPU build restates it), the launches.
//
// One iteration is refine_trials, the scorer's energy launch over the trial rows by their mask, refine_select:
//   refine_begin    a thread per pose: the state at the start (energy = the start energy, the steps, the counters);
//   refine_trials   a workgroup per pose: the K trial rows of an unfrozen pose and their `active` bytes (0 for a frozen pose,
//                   whose rows stay as they are);
//   refine_select   a wave per pose: the first maximum of its K energies, then pose, energy, steps, counters and history.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace ld {

constexpr int kRefineThreads = 256;     // 4 wave64: refine_select takes 4 poses a workgroup
constexpr int kRefineMaxPoseLen = 135;  // 7 + 64 + 64 (a scorer takes at most 64 modes a side)

// ld_refine_history's values below zero
constexpr int16_t kRefineHalved = -1, kRefineFrozen = -2, kRefineNotEvaluated = -3;

// The state of n poses, one array each (device pointers in a launch).
struct RefineState {
    double *energy = nullptr, *trans_step = nullptr, *rot_cos = nullptr, *rot_sin = nullptr, *nm_step = nullptr;
    uint32_t *halvings = nullptr, *accepted = nullptr, *evaluations = nullptr;
    uint8_t *frozen = nullptr;
};

struct RefineLaunch {
    size_t n_poses = 0;
    int pose_len = 0;        // 7 .. kRefineMaxPoseLen
    double *poses = nullptr; // row p at poses + p * stride; only its first pose_len doubles are read or written
    size_t stride = 0;
    RefineState state;
};

// --- the rule -----------------------------------------------------------------------------------------------------------

__host__ __device__ inline int refine_trial_count(int pose_len) { return 12 + 2 * (pose_len - 7); }

// Component `comp` (0 w, 1 x, 2 y, 3 z) of r q: Quaternion::mul, src/qt.rs:177-184, the same expression in the same order.
__host__ __device__ inline double refine_q_mul(const double r[4], const double q[4], int comp) {
    switch (comp) {
    case 0: return r[0] * q[0] - r[1] * q[1] - r[2] * q[2] - r[3] * q[3];
    case 1: return r[0] * q[1] + r[1] * q[0] + r[2] * q[3] - r[3] * q[2];
    case 2: return r[0] * q[2] - r[1] * q[3] + r[2] * q[0] + r[3] * q[1];
    default: return r[0] * q[3] + r[1] * q[2] - r[2] * q[1] + r[3] * q[0];
    }
}

// Element e of trial j of the pose `row` (pose_len doubles): the pose's own bits wherever the move does not reach.
__host__ __device__ inline double refine_trial_value(const double *row, int j, int e, double dt, double c, double s, double dn) {
    const bool minus = (j & 1) != 0;
    if (j < 6) {
        if (e != (j >> 1)) return row[e];
        return minus ? row[e] - dt : row[e] + dt;
    }
    if (j < 12) {
        if (e < 3 || e >= 7) return row[e];
        double r[4] = {c, 0.0, 0.0, 0.0};
        r[1 + ((j - 6) >> 1)] = minus ? -s : s;
        return refine_q_mul(r, row + 3, e - 3);
    }
    if (e != 7 + ((j - 12) >> 1)) return row[e];
    return minus ? row[e] - dn : row[e] + dn;
}

// A failure below the limit: IEEE add, multiply, divide and square root only.
__host__ __device__ inline void refine_halve(double *dt, double *c, double *s, double *dn) {
    *dt = *dt * 0.5;
    *dn = *dn * 0.5;
    const double c2 = sqrt((1.0 + *c) * 0.5);
    *s = *s / (2.0 * c2);
    *c = c2;
}

// Of two trials the larger energy wins, of equal energies the lower index.
__host__ __device__ inline bool refine_better(double ea, int ja, double eb, int jb) { return ea > eb || (ea == eb && ja < jb); }

// What refine_select does for one unfrozen pose once (e_best, j_best) is known; the history entry is returned.
__host__ __device__ inline int16_t refine_decide(const RefineLaunch &L, size_t p, double e_best, int j_best, uint32_t max_halvings) {
    const RefineState &S = L.state;
    double *row = L.poses + p * L.stride;
    S.evaluations[p] += (uint32_t)refine_trial_count(L.pose_len);
    if (e_best > S.energy[p]) {
        const double dt = S.trans_step[p], c = S.rot_cos[p], s = S.rot_sin[p], dn = S.nm_step[p];
        if (j_best >= 6 && j_best < 12) {
            double q[4];
            for (int k = 0; k < 4; k++) q[k] = refine_trial_value(row, j_best, 3 + k, dt, c, s, dn);
            for (int k = 0; k < 4; k++) row[3 + k] = q[k];
        } else {
            const int e = j_best < 6 ? (j_best >> 1) : 7 + ((j_best - 12) >> 1);
            row[e] = refine_trial_value(row, j_best, e, dt, c, s, dn);
        }
        S.energy[p] = e_best;
        S.accepted[p] += 1;
        return (int16_t)j_best;
    }
    if (S.halvings[p] < max_halvings) {
        S.halvings[p] += 1;
        refine_halve(&S.trans_step[p], &S.rot_cos[p], &S.rot_sin[p], &S.nm_step[p]);
        return kRefineHalved;
    }
    S.frozen[p] = 1;
    return kRefineFrozen;
}

// --- the launches -------------------------------------------------------------------------------------------------------

// The state of every pose at the start: energy[p] = start_energy[p] (device), the steps as given, halvings = accepted = 0,
// evaluations = 1, frozen = 0.
hipError_t launch_refine_begin(const RefineLaunch &L, const double *start_energy, double trans_step, double rot_cos, double rot_sin,
                               double nm_step, hipStream_t stream);
// trials: trial j of pose p at trials + (p * K + j) * trial_stride, its first pose_len doubles; active: n_poses x K bytes.
hipError_t launch_refine_trials(const RefineLaunch &L, double *trials, size_t trial_stride, uint8_t *active, hipStream_t stream);
// energies: n_poses x K (a frozen pose's row is not read); history: pose p's entry at history[p * history_stride].
hipError_t launch_refine_select(const RefineLaunch &L, const double *energies, uint32_t max_halvings, int16_t *history,
                                size_t history_stride, hipStream_t stream);

}  // namespace ld
