// refine.hpp -- the host object behind ld_scorer_refine (include/lightdock_hip.h "Local refinement"): the grow-only workspace
// of a pass, carved by host/refine_plan.hpp, and the passes of a call.  Reached through an `ld_scorer*`, which builds it on
// first use; the trial rows run through that scorer's energy_batch_device by their mask.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "device_memory.hpp"
#include "host/refine_plan.hpp"
#include "kernels/refine.hpp"
#include "lightdock_hip.h"

namespace ld {

class Scorer;

class Refiner {
   public:
    explicit Refiner(Scorer &scorer);
    Refiner(const Refiner &) = delete;
    Refiner &operator=(const Refiner &) = delete;
    ~Refiner();

    size_t last_slice() const { return last_slice_; }   // 0: no call yet
    double last_kernel_ms() const { return last_ms_; }
    uint64_t last_evaluations() const { return last_evaluations_; }

    // ld_scorer_refine: every refusal is thrown before anything is launched or written.  Synchronous on the scorer's stream.
    void run(const ld_refine_options &o, size_t n, const double *poses, size_t stride, double *poses_out, ld_refine_stats *stats_out,
             ld_refine_history *history_out);

   private:
    Scorer &scorer_;
    DeviceBuffer ws_;
    hipEvent_t start_ = nullptr, stop_ = nullptr;
    size_t last_slice_ = 0;
    double last_ms_ = 0.0;
    uint64_t last_evaluations_ = 0;
};

// ld_refine_trials / ld_refine_select: one launch of that kernel on the caller's arrays, on the null stream, synchronised.
void refine_trials_host(size_t n, size_t pose_len, const double *poses, size_t stride, const ld_refine_state &state, double *trials,
                        size_t trial_stride, uint8_t *active_out);
void refine_select_host(size_t n, size_t pose_len, double *poses, size_t stride, const ld_refine_state &state, const double *energies,
                        uint32_t max_halvings, ld_refine_history *history_out);

}  // namespace ld
