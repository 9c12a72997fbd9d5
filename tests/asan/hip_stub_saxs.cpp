// hip_stub_saxs.cpp -- TEST INFRASTRUCTURE for the sanitizer build of the host side (`make asan`, `make asan-saxs`): the
// launches of kernels/saxs.hpp, beside tests/asan/hip_stub.cpp which stands in for the HIP runtime and every other kernel.
// Device memory is host memory there, so ASan checks every extent below against what saxs.cpp allocated.  The launches do
// their kernels' work in plain C++ from the rule both sides share (saxs_pair_class, saxs_axis, saxs_d2, saxs_bin: host
// code too): posing and rounding by the kernel's own kernels/complex_rule.hpp, then every pair a < b in one loop --
// no tiles, no split, so a disagreement with the kernel's structure would show -- and the Debye sums in the stated order.
#include <cmath>
#include <cstring>
#include <vector>

#include "kernels/complex_rule.hpp"
#include "kernels/saxs.hpp"
#include "stub_access.hpp"

namespace ld {

hipError_t launch_saxs_pose(const ComplexDevice &m, const SaxsDevice &d, const double *poses, size_t stride, size_t n, int first,
                            int count, int4 *out, size_t out_stride, int *overflow, hipStream_t) {
    if (n == 0 || count <= 0) return hipSuccess;
    if (n > 65535 || first < 0 || first + count > d.n_part || out_stride < (size_t)count) return hipErrorInvalidValue;
    if (d.n_part_rec > d.n_part || d.n_part > m.n_rec + m.n_lig || d.n_part > kSaxsMaxAtoms) return hipErrorInvalidValue;
    peek_complex(m, poses, stride, n);
    peek(d.part_atom, (size_t)d.n_part);
    peek(d.part_class, (size_t)d.n_part);
    touch(out, (n - 1) * out_stride + count);
    peek(overflow, 1);   // set, never cleared, by the kernel
    for (int a = 0; a < d.n_part; a++) {
        const uint32_t atom = d.part_atom[a];
        if (atom >= (uint32_t)(m.n_rec + m.n_lig) || (a && atom <= d.part_atom[a - 1]) || (a < d.n_part_rec) != (atom < (uint32_t)m.n_rec))
            return hipErrorInvalidValue;
        if (d.part_class[a] >= kSaxsClasses) return hipErrorInvalidValue;
    }
    for (size_t i = 0; i < n; i++)
        for (int a = 0; a < count; a++) {
            int v[3];
            if (!posed_thousandths(m, poses + i * stride, d.part_atom[first + a], kComplexCoordBound, v)) *overflow = 1;
            out[i * out_stride + a] = make_int4(v[0], v[1], v[2], (int)d.part_class[first + a]);
        }
    return hipSuccess;
}

hipError_t launch_saxs_rows(const uint32_t *base, uint32_t *rows, size_t n, size_t row_words, hipStream_t) {
    if (base) peek(base, row_words);
    for (size_t i = 0; i < n; i++)
        for (size_t k = 0; k < row_words; k++) rows[i * row_words + k] = base ? base[k] : 0u;
    return hipSuccess;
}

hipError_t launch_saxs_histogram(const SaxsHistogram &h, size_t n, hipStream_t) {
    if (n == 0 || saxs_tile_pairs(h.n_atoms, h.first_b) <= 0) return hipSuccess;
    if (n > 65535 || h.splits < 1 || h.splits > saxs_tile_pairs(h.n_atoms, h.first_b) || h.bins < 1 || h.bins > kSaxsMaxBins) return hipErrorInvalidValue;
    if (h.width < (uint32_t)kSaxsMinWidth || h.width > (uint32_t)kSaxsMaxWidth || h.first_b < 0 || h.first_b > h.n_atoms) return hipErrorInvalidValue;
    if (h.atom_stride < (size_t)h.n_atoms || saxs_histogram_lds_bytes(h.bins) + kSaxsTile * sizeof(int4) > 160 * 1024) return hipErrorInvalidValue;   // a CU's LDS
    const size_t words = (size_t)kSaxsPairClasses * h.bins;
    peek(h.atoms, (n - 1) * h.atom_stride + h.n_atoms);
    peek(h.counts, n * words);   // initialised by the caller, added to
    peek(h.overflow, 1);
    for (size_t i = 0; i < n; i++) {
        const int4 *atoms = h.atoms + i * h.atom_stride;
        uint32_t *row = h.counts + i * words;
        for (int b = h.first_b > 1 ? h.first_b : 1; b < h.n_atoms; b++)
            for (int a = 0; a < b; a++) {
                const unsigned long long d2 = saxs_d2(saxs_axis(atoms[a].x - atoms[b].x), saxs_axis(atoms[a].y - atoms[b].y), saxs_axis(atoms[a].z - atoms[b].z));
                const uint32_t estimate = (uint32_t)(std::sqrt((double)d2) / (double)h.width);
                const uint32_t k = saxs_bin(d2, h.width, estimate);
                if (k < (uint32_t)h.bins) row[saxs_pair_class((uint32_t)atoms[a].w, (uint32_t)atoms[b].w) * h.bins + k]++;
                else *h.overflow = 1;
                if (((saxs_pair_fields((uint32_t)atoms[a].w) >> (5 * atoms[b].w)) & 31u) != saxs_pair_class((uint32_t)atoms[a].w, (uint32_t)atoms[b].w)) return hipErrorInvalidValue;
            }
    }
    return hipSuccess;
}

hipError_t launch_saxs_debye(const SaxsDebye &d, size_t n, hipStream_t) {
    if (n == 0) return hipSuccess;
    if (d.bins < 1 || d.bins > kSaxsMaxBins || d.n_q < 1 || d.n_q > kSaxsMaxQ) return hipErrorInvalidValue;
    const size_t words = (size_t)kSaxsPairClasses * d.bins;
    peek(d.counts, n * words);
    peek(d.sinc_t, (size_t)d.bins * d.n_q);
    peek(d.self, (size_t)d.n_q);
    peek(d.cross, (size_t)d.n_q * kSaxsPairClasses);
    touch(d.intensity, n * (size_t)d.n_q);
    for (size_t i = 0; i < n; i++)
        for (int j = 0; j < d.n_q; j++) {
            double I = d.self[j];
            for (int c = 0; c < kSaxsPairClasses; c++) {
                double G = 0.0;
                for (int k = 0; k < d.bins; k++) G = G + (double)d.counts[i * words + (size_t)c * d.bins + k] * d.sinc_t[(size_t)k * d.n_q + j];
                I = I + d.cross[(size_t)j * kSaxsPairClasses + c] * G;
            }
            d.intensity[i * (size_t)d.n_q + j] = I;
        }
    return hipSuccess;
}

}  // namespace ld
