// stub_access.hpp -- TEST INFRASTRUCTURE of the sanitizer build: how the stubs (tests/asan/hip_stub*.cpp) show ASan the extent of
// a buffer as a kernel indexes it.  Byte-wise, so that every element type serves (int4 too).
#pragma once

#include <cstddef>
#include <cstring>

#include "kernels/cluster.hpp"

namespace ld {

// The first and the last element of a buffer a kernel writes: both are cleared.
template <typename T>
static void touch(T *base, size_t count) {
    if (!count) return;
    std::memset(&base[0], 0, sizeof(T));
    std::memset(&base[count - 1], 0, sizeof(T));
}
// ... of a buffer a kernel reads, or one it updates in place whose content the stub needs: ASan checks an address the same for a
// read as for a write.
template <typename T>
static void peek(const T *base, size_t count) {
    if (!count) return;
    volatile unsigned char first = *reinterpret_cast<const unsigned char *>(&base[0]);
    volatile unsigned char last = reinterpret_cast<const unsigned char *>(&base[count - 1])[sizeof(T) - 1];
    (void)first;
    (void)last;
}

// What every posing kernel reads: the complex, and pose rows 0 .. n_poses - 1 (row i: poses + i * stride).
static inline void peek_complex(const ComplexDevice &m, const double *poses, size_t stride, size_t n_poses) {
    peek(m.rec_xyz, 3 * (size_t)m.n_rec);
    peek(m.lig_xyz, 3 * (size_t)m.n_lig);
    peek(m.rec_modes, (size_t)m.anm_rec * m.n_rec * 3);
    peek(m.lig_modes, (size_t)m.anm_lig * m.n_lig * 3);
    if (n_poses) peek(poses, (n_poses - 1) * stride + 7 + m.anm_rec + m.anm_lig);
}

}  // namespace ld
