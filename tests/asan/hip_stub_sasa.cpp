// hip_stub_sasa.cpp -- TEST INFRASTRUCTURE for the sanitizer build of the host side (`make asan`, `make asan-sasa`): the
// launch of kernels/sasa.hpp, beside tests/asan/hip_stub.cpp which stands in for the HIP runtime and every other kernel.
// Device memory is host memory there, so ASan checks every extent below against what complex.cpp allocated.  The launch
// does its kernel's work in plain C++ from the rule both sides share (sasa_offset, sasa_buried, kSasaDirections: host code
// too): posing and rounding by the kernel's own kernels/complex_rule.hpp, then every point of every atom against
// every atom whose box of reach holds it -- no grid, no list, so a disagreement with the kernel's structure would show.
#include <cmath>
#include <cstring>
#include <vector>

#include "kernels/complex_rule.hpp"
#include "kernels/sasa.hpp"
#include "stub_access.hpp"

namespace ld {

struct Atom {
    long long c[3];
    int E;
};

// The exposed points of atom a after the atoms [b0, b1) other than `self`; mask in, mask out (two words of 64 points).
static void bury(const std::vector<Atom> &atoms, size_t a, size_t b0, size_t b1, unsigned long long ex[2]) {
    const Atom &me = atoms[a];
    for (size_t b = b0; b < b1; b++) {
        if (b == a) continue;
        const Atom &o = atoms[b];
        const long long reach = me.E + o.E + kSasaSlack;
        long long rel[3];
        bool near = true;
        for (int k = 0; k < 3; k++) {
            rel[k] = o.c[k] - me.c[k];
            near = near && rel[k] <= reach && rel[k] >= -reach;
        }
        if (!near) continue;   // a point is within E_a + 1 of c_a: only a speed-up
        for (int p = 0; p < kSasaPoints; p++) {
            if (!(ex[p >> 6] >> (p & 63) & 1)) continue;
            if (sasa_buried(sasa_offset(me.E, kSasaDirections[p][0]), sasa_offset(me.E, kSasaDirections[p][1]),
                            sasa_offset(me.E, kSasaDirections[p][2]), (int)rel[0], (int)rel[1], (int)rel[2], o.E * o.E))
                ex[p >> 6] &= ~(1ull << (p & 63));
        }
    }
}

hipError_t launch_complex_sasa(const ComplexDevice &m, const SasaDevice &d, const double *poses, size_t stride, size_t n, size_t slots,
                               void *ws, unsigned long long *sums, uint8_t *free_counts, uint8_t *bound_counts, int *overflow,
                               hipStream_t) {
    if (slots < 1 || slots > (size_t)kSasaSlots || slots > n) return hipErrorInvalidValue;
    if (d.probe < 0 || d.probe > kSasaMaxProbe || d.e_max < d.probe || d.e_max > kSasaMaxRadius + kSasaMaxProbe) return hipErrorInvalidValue;
    if (d.n_part_rec < 1 || d.n_part_rec >= d.n_part || d.n_part > d.n_atoms || d.n_atoms != m.n_rec + m.n_lig) return hipErrorInvalidValue;
    if ((free_counts == nullptr) != (bound_counts == nullptr)) return hipErrorInvalidValue;
    peek_complex(m, poses, stride, n);
    peek(d.part_atom, (size_t)d.n_part);
    peek(d.part_radius, (size_t)d.n_part);
    touch(static_cast<char *>(ws), slots * sasa_slot_bytes(d.n_part));   // ws + blockIdx * sasa_slot_bytes
    touch(sums, n * 4);
    peek(overflow, 1);   // set, never cleared, by the kernel
    for (int a = 0; a < d.n_part; a++) {
        const uint32_t atom = d.part_atom[a], R = d.part_radius[a];
        if (atom >= (uint32_t)d.n_atoms || (a && atom <= d.part_atom[a - 1]) || (a < d.n_part_rec) != (atom < (uint32_t)m.n_rec))
            return hipErrorInvalidValue;
        if (R < 1 || (int)R + d.probe > d.e_max) return hipErrorInvalidValue;
    }
    std::vector<Atom> atoms((size_t)d.n_part);
    for (size_t i = 0; i < n; i++) {
        const double *row = poses + i * stride;
        for (int a = 0; a < d.n_part; a++) {
            int v[3];
            if (!posed_thousandths(m, row, d.part_atom[a], kComplexCoordBound, v)) *overflow = 1;
            for (int k = 0; k < 3; k++) atoms[a].c[k] = v[k];
            atoms[a].E = (int)d.part_radius[a] + d.probe;
        }
        unsigned long long acc[4] = {0, 0, 0, 0};
        for (int a = 0; a < d.n_part; a++) {
            const bool lig = a >= d.n_part_rec;
            const size_t own0 = lig ? d.n_part_rec : 0, own1 = lig ? d.n_part : d.n_part_rec;
            unsigned long long ex[2] = {~0ull, ~0ull};
            bury(atoms, a, own0, own1, ex);
            const int n_free = __builtin_popcountll(ex[0]) + __builtin_popcountll(ex[1]);
            bury(atoms, a, lig ? 0 : d.n_part_rec, lig ? d.n_part_rec : d.n_part, ex);
            const int n_bound = __builtin_popcountll(ex[0]) + __builtin_popcountll(ex[1]);
            const unsigned long long E2 = (unsigned long long)atoms[a].E * atoms[a].E;
            acc[lig ? 2 : 0] += E2 * n_free;
            acc[lig ? 3 : 1] += E2 * n_bound;
            if (free_counts) {
                const size_t at = i * (size_t)d.n_atoms + d.part_atom[a];
                free_counts[at] = (uint8_t)n_free;
                bound_counts[at] = (uint8_t)n_bound;
            }
        }
        std::memcpy(sums + i * 4, acc, sizeof acc);
    }
    return hipSuccess;
}

}  // namespace ld
