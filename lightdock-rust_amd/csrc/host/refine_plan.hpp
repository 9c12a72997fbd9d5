// refine_plan.hpp -- the arithmetic of a local refinement call (include/lightdock_hip.h "Local refinement"): the trials of
// a pose, the poses of a pass, the bytes of a pass's workspace and every refusal that is a matter of sizes or options.
// Host only, no HIP: ld_refine_plan exposes it, refine.cpp carves its workspace by it.
#pragma once

#include <cstddef>
#include <cstdint>

#include "lightdock_hip.h"

namespace ld {

constexpr size_t kRefinePoseLenMax = 135;                 // 7 + 64 + 64: a scorer takes at most 64 modes a side
constexpr size_t kRefineDefaultRows = (size_t)1 << 16;    // trial rows of a pass by default: slice = 65 536 / K
constexpr size_t kRefineMaxRows = (size_t)1 << 22;        // ... and at most, where the caller names the slice

struct RefinePlan {
    size_t trials = 0;   // K = 12 + 2 (pose_len - 7)
    size_t slice = 0;    // poses per pass
    size_t cap = 0;      // poses the workspace is carved for: min(slice, n)
    // the workspace, in this order (8-byte, 4-byte, 2-byte, 1-byte elements): counts of elements
    size_t pose_doubles = 0, trial_doubles = 0, energy_doubles = 0, state_doubles = 0;   // state: start energy + 5 arrays of cap
    size_t state_words = 0;      // 3 arrays of cap uint32
    size_t history_entries = 0;  // cap x iterations int16
    size_t active_bytes = 0, frozen_bytes = 0;
    size_t workspace_bytes = 0;
};

// Throws Error(LD_ERR_INVALID): pose_len outside 7 .. 135, stride < pose_len, iterations == 0, slice_request x K beyond
// kRefineMaxRows, or any of n x stride x 8, n x pose_len x 8, n x iterations x 2 and the workspace beyond a size_t.
RefinePlan refine_plan(size_t pose_len, size_t n, size_t stride, size_t iterations, size_t slice_request);

// Throws Error(LD_ERR_INVALID): iterations == 0, a step that is not finite and > 0, rot_step > pi.
void refine_check_options(const ld_refine_options &o);

}  // namespace ld
