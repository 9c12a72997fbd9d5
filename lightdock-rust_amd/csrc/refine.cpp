#include "refine.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "scorer.hpp"

namespace ld {

Refiner::Refiner(Scorer &scorer) : scorer_(scorer) {
    hip_check(hipEventCreate(&start_), "hipEventCreate");
    hip_check(hipEventCreate(&stop_), "hipEventCreate");
}

Refiner::~Refiner() {
    if (start_) (void)hipEventDestroy(start_);
    if (stop_) (void)hipEventDestroy(stop_);
}

void Refiner::run(const ld_refine_options &o, size_t n, const double *poses, size_t stride, double *poses_out, ld_refine_stats *stats_out,
                  ld_refine_history *history_out) {
    refine_check_options(o);
    const size_t pose_len = scorer_.pose_len(), iterations = o.iterations;
    const RefinePlan plan = refine_plan(pose_len, n, stride, iterations, o.slice_poses);
    if (n == 0) return;
    if (!poses || !poses_out) throw Error(LD_ERR_INVALID, "ld_scorer_refine: poses missing");

    // the workspace of a pass, carved for `cap` poses in the plan's order
    const size_t cap = plan.cap, K = plan.trials;
    ws_.reserve(plan.workspace_bytes);
    double *d = static_cast<double *>(ws_.ptr);
    double *d_poses = d;
    d += plan.pose_doubles;
    double *d_trials = d;
    d += plan.trial_doubles;
    double *d_energies = d;
    d += plan.energy_doubles;
    double *d_before = d;
    d += cap;
    RefineLaunch L;
    L.pose_len = (int)pose_len;
    L.poses = d_poses;
    L.stride = pose_len;
    L.state.energy = d, d += cap;
    L.state.trans_step = d, d += cap;
    L.state.rot_cos = d, d += cap;
    L.state.rot_sin = d, d += cap;
    L.state.nm_step = d, d += cap;
    uint32_t *u = reinterpret_cast<uint32_t *>(d);
    L.state.halvings = u, u += cap;
    L.state.accepted = u, u += cap;
    L.state.evaluations = u, u += cap;
    int16_t *d_history = reinterpret_cast<int16_t *>(u);
    uint8_t *d_active = reinterpret_cast<uint8_t *>(d_history + plan.history_entries);
    L.state.frozen = d_active + plan.active_bytes;
    // no allocation inside the loop: the scorer's workspace for the largest launch of a pass
    scorer_.prepare_batch(cap * K);

    const double rot_cos = std::cos(o.rot_step / 2), rot_sin = std::sin(o.rot_step / 2);
    const hipStream_t stream = scorer_.stream();
    std::vector<double> stage(cap * pose_len), h_before(cap), h_after(cap);
    std::vector<uint32_t> h_words(3 * cap);
    std::vector<uint8_t> h_frozen(cap);
    last_slice_ = plan.slice;
    last_ms_ = 0.0;
    last_evaluations_ = 0;
    for (size_t first = 0; first < n; first += plan.slice) {
        const size_t m = std::min(plan.slice, n - first);
        for (size_t p = 0; p < m; p++) std::memcpy(&stage[p * pose_len], poses + (first + p) * stride, pose_len * sizeof(double));
        hip_check(hipMemcpyAsync(d_poses, stage.data(), m * pose_len * sizeof(double), hipMemcpyHostToDevice, stream), "hipMemcpy H2D");
        L.n_poses = m;
        hip_check(hipEventRecord(start_, stream), "hipEventRecord");
        scorer_.energy_batch_device(m, d_poses, pose_len, nullptr, d_before, nullptr);
        hip_check(launch_refine_begin(L, d_before, o.trans_step, rot_cos, rot_sin, o.nm_step, stream), "launch refine_begin");
        for (size_t it = 0; it < iterations; it++) {
            hip_check(launch_refine_trials(L, d_trials, pose_len, d_active, stream), "launch refine_trials");
            scorer_.energy_batch_device(m * K, d_trials, pose_len, d_active, d_energies, nullptr);
            hip_check(launch_refine_select(L, d_energies, o.max_halvings, d_history + it, iterations, stream), "launch refine_select");
        }
        hip_check(hipEventRecord(stop_, stream), "hipEventRecord");
        hip_check(hipMemcpyAsync(poses_out + first * pose_len, d_poses, m * pose_len * sizeof(double), hipMemcpyDeviceToHost, stream), "hipMemcpy D2H");
        hip_check(hipMemcpyAsync(h_words.data(), L.state.halvings, 3 * cap * sizeof(uint32_t), hipMemcpyDeviceToHost, stream), "hipMemcpy D2H");
        if (stats_out) {
            hip_check(hipMemcpyAsync(h_before.data(), d_before, m * sizeof(double), hipMemcpyDeviceToHost, stream), "hipMemcpy D2H");
            hip_check(hipMemcpyAsync(h_after.data(), L.state.energy, m * sizeof(double), hipMemcpyDeviceToHost, stream), "hipMemcpy D2H");
            hip_check(hipMemcpyAsync(h_frozen.data(), L.state.frozen, m, hipMemcpyDeviceToHost, stream), "hipMemcpy D2H");
        }
        if (history_out)
            hip_check(hipMemcpyAsync(history_out + first * iterations, d_history, m * iterations * sizeof(int16_t), hipMemcpyDeviceToHost, stream),
                      "hipMemcpy D2H");
        hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
        float ms = 0.f;
        hip_check(hipEventElapsedTime(&ms, start_, stop_), "hipEventElapsedTime");
        last_ms_ += (double)ms;
        for (size_t p = 0; p < m; p++) {
            last_evaluations_ += h_words[2 * cap + p];
            if (!stats_out) continue;
            ld_refine_stats &st = stats_out[first + p];
            st.energy_before = h_before[p];
            st.energy_after = h_after[p];
            st.halvings = h_words[p];
            st.accepted = h_words[cap + p];
            st.evaluations = h_words[2 * cap + p];
            st.frozen = h_frozen[p];
        }
    }
}

// ---------------------------------------------------------------------------------------
// The two kernels on caller-given state
// ---------------------------------------------------------------------------------------
namespace {

// The caller's state and poses on the device for one launch.
struct DeviceState {
    DeviceBuffer doubles, words, frozen, poses;
    size_t n = 0;
    RefineLaunch launch(size_t n_poses, size_t pose_len, const double *h_poses, size_t stride, const ld_refine_state &s) {
        n = n_poses;
        if (pose_len < 7 || pose_len > kRefinePoseLenMax) throw Error(LD_ERR_INVALID, "ld_refine: pose length outside 7 .. 135");
        if (stride < pose_len) throw Error(LD_ERR_INVALID, "ld_refine: stride below the pose length");
        if (!h_poses || !s.energy || !s.trans_step || !s.rot_cos || !s.rot_sin || !s.nm_step || !s.halvings || !s.accepted || !s.evaluations ||
            !s.frozen)
            throw Error(LD_ERR_INVALID, "ld_refine: null argument");
        if (n > ((size_t)1 << 22) / (12 + 2 * (pose_len - 7)) || stride > ((size_t)1 << 20)) throw Error(LD_ERR_INVALID, "ld_refine: more than 2^22 trial rows");
        doubles.reserve(5 * n * sizeof(double));
        words.reserve(3 * n * sizeof(uint32_t));
        frozen.reserve(n);
        poses.reserve(n * stride * sizeof(double));
        RefineLaunch L;
        L.n_poses = n;
        L.pose_len = (int)pose_len;
        L.poses = static_cast<double *>(poses.ptr);
        L.stride = stride;
        double *d = static_cast<double *>(doubles.ptr);
        uint32_t *u = static_cast<uint32_t *>(words.ptr);
        L.state.energy = d, L.state.trans_step = d + n, L.state.rot_cos = d + 2 * n, L.state.rot_sin = d + 3 * n, L.state.nm_step = d + 4 * n;
        L.state.halvings = u, L.state.accepted = u + n, L.state.evaluations = u + 2 * n;
        L.state.frozen = static_cast<uint8_t *>(frozen.ptr);
        const double *hd[5] = {s.energy, s.trans_step, s.rot_cos, s.rot_sin, s.nm_step};
        const uint32_t *hu[3] = {s.halvings, s.accepted, s.evaluations};
        for (int k = 0; k < 5; k++) hip_check(hipMemcpy(d + k * n, hd[k], n * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy H2D");
        for (int k = 0; k < 3; k++) hip_check(hipMemcpy(u + k * n, hu[k], n * sizeof(uint32_t), hipMemcpyHostToDevice), "hipMemcpy H2D");
        hip_check(hipMemcpy(frozen.ptr, s.frozen, n, hipMemcpyHostToDevice), "hipMemcpy H2D");
        hip_check(hipMemcpy(poses.ptr, h_poses, n * stride * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy H2D");
        return L;
    }
    void download(const RefineLaunch &L, double *h_poses, const ld_refine_state &s) {
        double *hd[5] = {s.energy, s.trans_step, s.rot_cos, s.rot_sin, s.nm_step};
        uint32_t *hu[3] = {s.halvings, s.accepted, s.evaluations};
        for (int k = 0; k < 5; k++) hip_check(hipMemcpy(hd[k], L.state.energy + k * n, n * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy D2H");
        for (int k = 0; k < 3; k++) hip_check(hipMemcpy(hu[k], L.state.halvings + k * n, n * sizeof(uint32_t), hipMemcpyDeviceToHost), "hipMemcpy D2H");
        hip_check(hipMemcpy(s.frozen, L.state.frozen, n, hipMemcpyDeviceToHost), "hipMemcpy D2H");
        hip_check(hipMemcpy(h_poses, L.poses, n * L.stride * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy D2H");
    }
};

}  // namespace

void refine_trials_host(size_t n, size_t pose_len, const double *poses, size_t stride, const ld_refine_state &state, double *trials,
                        size_t trial_stride, uint8_t *active_out) {
    if (n == 0) return;
    if (!trials || !active_out) throw Error(LD_ERR_INVALID, "ld_refine_trials: null argument");
    if (trial_stride < pose_len || trial_stride > ((size_t)1 << 20)) throw Error(LD_ERR_INVALID, "ld_refine_trials: trial stride below the pose length");
    DeviceState dev;
    const RefineLaunch L = dev.launch(n, pose_len, poses, stride, state);
    const size_t rows = n * (size_t)refine_trial_count((int)pose_len);
    DeviceBuffer d_trials, d_active;
    d_trials.reserve(rows * trial_stride * sizeof(double));
    d_active.reserve(rows);
    hip_check(hipMemcpy(d_trials.ptr, trials, rows * trial_stride * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy H2D");
    hip_check(launch_refine_trials(L, static_cast<double *>(d_trials.ptr), trial_stride, static_cast<uint8_t *>(d_active.ptr), nullptr), "launch refine_trials");
    hip_check(hipStreamSynchronize(nullptr), "hipStreamSynchronize");
    hip_check(hipMemcpy(trials, d_trials.ptr, rows * trial_stride * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy D2H");
    hip_check(hipMemcpy(active_out, d_active.ptr, rows, hipMemcpyDeviceToHost), "hipMemcpy D2H");
}

void refine_select_host(size_t n, size_t pose_len, double *poses, size_t stride, const ld_refine_state &state, const double *energies,
                        uint32_t max_halvings, ld_refine_history *history_out) {
    if (n == 0) return;
    if (!energies || !history_out) throw Error(LD_ERR_INVALID, "ld_refine_select: null argument");
    DeviceState dev;
    const RefineLaunch L = dev.launch(n, pose_len, poses, stride, state);
    const size_t rows = n * (size_t)refine_trial_count((int)pose_len);
    DeviceBuffer d_energies, d_history;
    d_energies.reserve(rows * sizeof(double));
    d_history.reserve(n * sizeof(int16_t));
    hip_check(hipMemcpy(d_energies.ptr, energies, rows * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy H2D");
    hip_check(launch_refine_select(L, static_cast<const double *>(d_energies.ptr), max_halvings, static_cast<int16_t *>(d_history.ptr), 1, nullptr),
              "launch refine_select");
    hip_check(hipStreamSynchronize(nullptr), "hipStreamSynchronize");
    dev.download(L, poses, state);
    hip_check(hipMemcpy(history_out, d_history.ptr, n * sizeof(int16_t), hipMemcpyDeviceToHost), "hipMemcpy D2H");
}

}  // namespace ld
