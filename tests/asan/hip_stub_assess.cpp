// hip_stub_assess.cpp -- TEST INFRASTRUCTURE for the sanitizer build of the host side (`make asan`, `make asan-assess`):
// the launches of kernels/assess.hpp, beside tests/asan/hip_stub.cpp which stands in for the HIP runtime and every other
// kernel.  Device memory is host memory there, so ASan checks every extent below against what complex.cpp allocated.
//   launch_complex_assess_sums touches both ends of every buffer the kernel reads or writes, the extents from the launch
//     arguments as assess.hip indexes them, walks the host-made lists whole (ascending used atoms, native ranges inside
//     the used list), and leaves for every pose the words of a model that IS the reference moved by (1, 2, 3) A;
//   launch_complex_assess_solve runs the real f64 arithmetic (assess_solve_pose is host code too) under UBSan.
#include <cstring>

#include "kernels/assess.hpp"
#include "stub_access.hpp"

namespace ld {

static void add_atom(long long *w, const long long m[3], const long long r[3]) {
    for (int a = 0; a < 3; a++) {
        w[a] += m[a];
        w[3] += m[a] * m[a];
        for (int b = 0; b < 3; b++) w[4 + 3 * a + b] += m[a] * r[b];
    }
}

hipError_t launch_complex_assess_sums(const ComplexDevice &m, const AssessDevice &d, const double *poses, size_t stride, size_t n,
                                      uint32_t C2, size_t slots, int4 *atoms_ws, long long *sums, int *overflow, hipStream_t) {
    if (slots < 1 || slots > (size_t)kAssessSlots || slots > n) return hipErrorInvalidValue;
    if (C2 < 1 || C2 > 900000000u) return hipErrorInvalidValue;   // C <= 30000: the clamped 32-bit test
    if (d.n_used < 1 || (size_t)d.n_used > kAssessMaxUsed || d.n_used_rec < 0 || d.n_used_rec > d.n_used || d.n_native < 1)
        return hipErrorInvalidValue;
    peek_complex(m, poses, stride, n);
    peek(d.used_atom, (size_t)d.n_used);
    peek(d.used_ref, (size_t)d.n_used);
    peek(d.native, (size_t)d.n_native);
    long long own[kAssessWords] = {};
    for (int u = 0; u < d.n_used; u++) {
        const uint32_t atom = d.used_atom[u];
        if (atom >= (uint32_t)(m.n_rec + m.n_lig) || (u && atom <= d.used_atom[u - 1])) return hipErrorInvalidValue;
        if ((u < d.n_used_rec) != (atom < (uint32_t)m.n_rec)) return hipErrorInvalidValue;
        const int4 ref = d.used_ref[u];
        if (abs(ref.x) > kAssessBound || abs(ref.y) > kAssessBound || abs(ref.z) > kAssessBound || (ref.w & ~3) || ref.w == 2)
            return hipErrorInvalidValue;
        const long long r[3] = {ref.x, ref.y, ref.z}, moved[3] = {r[0] + 1000, r[1] + 2000, r[2] + 3000};
        if (ref.w & 1) add_atom(own + (u < d.n_used_rec ? kAssessRec : kAssessLig), moved, r);
        if (ref.w & 2) add_atom(own + kAssessInt, moved, r);
    }
    for (int p = 0; p < d.n_native; p++) {
        const int4 pr = d.native[p];   // [x, y) in the receptor's used atoms, [z, w) in the ligand's
        if (pr.x < 0 || pr.x >= pr.y || pr.y > d.n_used_rec || pr.z < d.n_used_rec || pr.z >= pr.w || pr.w > d.n_used)
            return hipErrorInvalidValue;
    }
    own[kAssessKept] = d.n_native;
    touch(atoms_ws, slots * (size_t)d.n_used);   // atoms_ws + blockIdx * n_used
    touch(sums, n * kAssessWords);
    for (size_t i = 0; i < n; i++) std::memcpy(sums + i * kAssessWords, own, sizeof own);
    peek(overflow, 1);   // set, never cleared, by the kernel
    return hipSuccess;
}

hipError_t launch_complex_assess_solve(const AssessSolve &k, const long long *sums, size_t n, uint32_t *kept, double *lrmsd,
                                       double *irmsd, hipStream_t) {
    if (k.n_rec < 3 || k.n_lig < 1 || k.n_int < 3) return hipErrorInvalidValue;
    peek(sums, n * kAssessWords);
    touch(kept, n);
    touch(lrmsd, n);
    touch(irmsd, n);
    for (size_t i = 0; i < n; i++) {
        assess_solve_pose(k, sums + i * kAssessWords, &lrmsd[i], &irmsd[i]);
        kept[i] = (uint32_t)sums[i * kAssessWords + kAssessKept];
    }
    return hipSuccess;
}

}  // namespace ld
