// hip_stub_sasa.cpp -- TEST INFRASTRUCTURE for the sanitizer build of the host side (`make asan`, `make asan-sasa`): the
// launch of kernels/sasa.hpp, beside tests/asan/hip_stub.cpp which stands in for the HIP runtime and every other kernel.
// Device memory is host memory there, so ASan checks every extent below against what complex.cpp allocated.  The launch
// does its kernel's work in plain C++ from the rule both sides share (sasa_offset, sasa_buried, kSasaDirections: host code
// too): posing and rounding restated in f64 with the kernel's operation order, then every point of every atom against
// every atom whose box of reach holds it -- no grid, no list, so a disagreement with the kernel's structure would show.
#include <cmath>
#include <cstring>
#include <vector>

#include "kernels/sasa.hpp"

namespace ld {

template <typename T>
static void touch(T *base, size_t count) {
    if (!count) return;
    std::memset(&base[0], 0, sizeof(T));
    std::memset(&base[count - 1], 0, sizeof(T));
}
template <typename T>
static void peek(const T *base, size_t count) {
    if (!count) return;
    volatile unsigned char first = *reinterpret_cast<const unsigned char *>(&base[0]);
    volatile unsigned char last = reinterpret_cast<const unsigned char *>(&base[count - 1])[sizeof(T) - 1];
    (void)first;
    (void)last;
}

// complex_pose.hpp's pose_atom and thousandths, on the host
static void pose_atom_host(const ComplexDevice &m, const double *row, uint32_t atom, double out[3]) {
    if ((int)atom < m.n_rec) {
        for (int c = 0; c < 3; c++) out[c] = m.rec_xyz[3 * (size_t)atom + c];
        for (int k = 0; k < m.anm_rec; k++)
            for (int c = 0; c < 3; c++) out[c] += m.rec_modes[((size_t)k * m.n_rec + atom) * 3 + c] * row[7 + k];
        return;
    }
    const uint32_t a = atom - (uint32_t)m.n_rec;
    double v[3];
    for (int c = 0; c < 3; c++) v[c] = m.lig_xyz[3 * (size_t)a + c];
    for (int k = 0; k < m.anm_lig; k++)
        for (int c = 0; c < 3; c++) v[c] += m.lig_modes[((size_t)k * m.n_lig + a) * 3 + c] * row[7 + m.anm_rec + k];
    const double qw = row[3], qx = row[4], qy = row[5], qz = row[6], vx = v[0], vy = v[1], vz = v[2];
    const double aw = qw * 0.0 - qx * vx - qy * vy - qz * vz;
    const double ax = qw * vx + qx * 0.0 + qy * vz - qz * vy;
    const double ay = qw * vy - qx * vz + qy * 0.0 + qz * vx;
    const double az = qw * vz + qx * vy - qy * vx + qz * 0.0;
    const double n2 = qw * qw + qx * qx + qy * qy + qz * qz;
    const double bw = qw / n2, bx = -qx / n2, by = -qy / n2, bz = -qz / n2;
    out[0] = aw * bx + ax * bw + ay * bz - az * by + row[0];
    out[1] = aw * by - ax * bz + ay * bw + az * bx + row[1];
    out[2] = aw * bz + ax * by - ay * bx + az * bw + row[2];
}

static double thousandths_host(double x) {
    const double p = x * 1000.0, e = std::fma(x, 1000.0, -p), f = std::floor(p);
    if (p - f == 0.5) {
        if (e > 0.0) return f + 1.0;
        if (e < 0.0) return f;
    }
    return std::rint(p);
}

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
    peek(m.rec_xyz, 3 * (size_t)m.n_rec);
    peek(m.lig_xyz, 3 * (size_t)m.n_lig);
    peek(m.rec_modes, (size_t)m.anm_rec * m.n_rec * 3);
    peek(m.lig_modes, (size_t)m.anm_lig * m.n_lig * 3);
    peek(poses, (n - 1) * stride + 7 + m.anm_rec + m.anm_lig);   // row i: poses + i * stride
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
            double p[3];
            pose_atom_host(m, row, d.part_atom[a], p);
            for (int k = 0; k < 3; k++) {
                const double c = thousandths_host(p[k]);
                if (!(std::fabs(c) <= 1.0e9)) *overflow = 1;
                atoms[a].c[k] = (long long)std::fmax(-1.0e9, std::fmin(1.0e9, c));
            }
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
