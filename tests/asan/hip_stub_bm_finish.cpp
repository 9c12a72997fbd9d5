// hip_stub_bm_finish.cpp -- TEST INFRASTRUCTURE for the sanitizer build of the host side: the launch of dfire_bm_finish
// (kernels/dfire_bm.hpp), beside tests/asan/hip_stub.cpp which stands in for the HIP runtime and the other block-major launches.
// Device memory is host memory there, so ASan checks the extents below against what the scorer allocated.  Like
// launch_finish_kernel's stand-in it writes 0.0 for every pose of the batch the mask does not exclude (the stand-in of the GSO
// kernel fills no list of moved glowworms, so the list is not followed).
#include "kernels/dfire_bm.hpp"

namespace ld {

hipError_t launch_bm_finish(const BmLaunch &t, hipStream_t) {
    if (!t.n_poses) return hipSuccess;
    if (!t.energies || t.count_mode || t.first != 0 || t.n_poses > t.cap) return hipErrorInvalidValue;
    const size_t flag_words = (size_t)(t.m.rec_flag_words + t.m.lig.flag_words);
    volatile long long sum = t.tile_sum[(size_t)(t.m.lig.n_tiles - 1) * t.cap + t.n_poses - 1] + t.exact_fix[t.n_poses - 1];   // [ligand tile][row], [row]
    (void)sum;
    if (flag_words) {
        volatile uint32_t word = t.flags[t.n_poses * flag_words - 1];   // [pose][rec words + lig words]
        (void)word;
    }
    for (int k = 0; k < t.tail.n_membrane; k++) {
        volatile uint32_t slot = t.tail.membrane_slots[k];
        (void)slot;
    }
    for (size_t pose = 0; pose < t.n_poses; pose++)
        if (!t.active || t.active[pose]) t.energies[pose] = 0.0;   // the output buffer really has n_poses doubles
    return hipSuccess;
}

}  // namespace ld
