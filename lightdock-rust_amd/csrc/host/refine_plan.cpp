#include "host/refine_plan.hpp"

#include <cmath>
#include <limits>
#include <string>

#include "host/error.hpp"

namespace ld {

namespace {

size_t mul(size_t a, size_t b, const char *what) {
    if (b != 0 && a > std::numeric_limits<size_t>::max() / b) throw Error(LD_ERR_INVALID, std::string("ld_refine: ") + what + " overflows");
    return a * b;
}
size_t add(size_t a, size_t b) {
    if (a > std::numeric_limits<size_t>::max() - b) throw Error(LD_ERR_INVALID, "ld_refine: the workspace overflows");
    return a + b;
}

}  // namespace

RefinePlan refine_plan(size_t pose_len, size_t n, size_t stride, size_t iterations, size_t slice_request) {
    if (pose_len < 7 || pose_len > kRefinePoseLenMax) throw Error(LD_ERR_INVALID, "ld_refine: pose length outside 7 .. 135");
    if (stride < pose_len) throw Error(LD_ERR_INVALID, "ld_refine: stride below the pose length");
    if (iterations == 0) throw Error(LD_ERR_INVALID, "ld_refine: iterations == 0");
    RefinePlan p;
    p.trials = 12 + 2 * (pose_len - 7);
    if (slice_request > kRefineMaxRows / p.trials) throw Error(LD_ERR_INVALID, "ld_refine: slice_poses x K beyond 2^22 trial rows");
    p.slice = slice_request ? slice_request : kRefineDefaultRows / p.trials;
    // what the caller's arrays hold
    mul(mul(n, stride, "n x stride"), sizeof(double), "n x stride");
    mul(mul(n, pose_len, "n x pose_len"), sizeof(double), "n x pose_len");
    mul(mul(n, iterations, "n x iterations"), sizeof(int16_t), "n x iterations");
    p.cap = n < p.slice ? n : p.slice;
    const size_t rows = p.cap * p.trials;   // <= 2^22
    p.pose_doubles = p.cap * pose_len;
    p.trial_doubles = rows * pose_len;
    p.energy_doubles = rows;
    p.state_doubles = 6 * p.cap;
    p.state_words = 3 * p.cap;
    p.history_entries = mul(p.cap, iterations, "slice x iterations");
    p.active_bytes = rows;
    p.frozen_bytes = p.cap;
    const size_t doubles = p.pose_doubles + p.trial_doubles + p.energy_doubles + p.state_doubles;   // < 2^22 x 138
    size_t bytes = doubles * sizeof(double) + p.state_words * sizeof(uint32_t);
    bytes = add(bytes, mul(p.history_entries, sizeof(int16_t), "slice x iterations"));
    bytes = add(bytes, p.active_bytes + p.frozen_bytes);
    p.workspace_bytes = bytes;
    return p;
}

void refine_check_options(const ld_refine_options &o) {
    if (o.iterations == 0) throw Error(LD_ERR_INVALID, "ld_scorer_refine: iterations == 0");
    const double steps[3] = {o.trans_step, o.rot_step, o.nm_step};
    for (double step : steps)
        if (!std::isfinite(step) || !(step > 0.0)) throw Error(LD_ERR_INVALID, "ld_scorer_refine: a step that is not finite and > 0");
    if (o.rot_step > 3.14159265358979323846) throw Error(LD_ERR_INVALID, "ld_scorer_refine: rot_step beyond pi");
}

}  // namespace ld
