// decompose_pair.hpp -- the arithmetic of one pose and one atom pair of the energy decomposition (kernels/decompose.hpp), as
// plain functions the kernels AND the sanitizer build's stand-in launches (tests/asan/hip_stub_decompose.cpp) compile: the
// definition of include/lightdock_hip.h, "Energy decomposition", operation for operation.  Built with -ffp-contract=off.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define LD_PAIR_FN __host__ __device__ __forceinline__
#else
#define LD_PAIR_FN inline
#endif

namespace ld {
namespace decompose {

struct Quat {
    double w, x, y, z;
};

// Hamilton product in the reference's term order, src/qt.rs:174-185
LD_PAIR_FN Quat qmul(const Quat &a, const Quat &b) {
    Quat r;
    r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
    r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
    r.y = a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x;
    r.z = a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w;
    return r;
}

// conj(q) / |q|^2, src/qt.rs:48-50
LD_PAIR_FN Quat qinverse(const Quat &q) {
    const double n2 = q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z;
    Quat r;
    r.w = q.w / n2;
    r.x = -q.x / n2;
    r.y = -q.y / n2;
    r.z = -q.z / n2;
    return r;
}

// One atom posed: the ligand rotated and translated (src/dfire.rs:282-290), then either side's ANM terms in ascending mode
// order (:292-320).  modes: [mode][xyz][n_pad]; row: the pose; ext: its extents for this side.
LD_PAIR_FN void pose_atom(bool ligand, const double *row, double x, double y, double z, int num_anm, const double *modes, size_t n_pad,
                          size_t atom, const double *ext, double out[3]) {
    double px = x, py = y, pz = z;
    if (ligand) {
        const Quat q{row[3], row[4], row[5], row[6]};
        const Quat r = qmul(qmul(q, Quat{0.0, x, y, z}), qinverse(q));
        px = r.x + row[0];
        py = r.y + row[1];
        pz = r.z + row[2];
    }
    for (int k = 0; k < num_anm; k++) {
        const double c = ext[k];
        const double *m = modes + (size_t)k * 3 * n_pad;
        px += m[atom] * c;
        py += m[n_pad + atom] * c;
        pz += m[2 * n_pad + atom] * c;
    }
    out[0] = px;
    out[1] = py;
    out[2] = pz;
}

// (x1 - la[0])^2 + (y1 - la[1])^2 + (z1 - la[2])^2, src/dfire.rs:331-333: receptor minus ligand, left to right
LD_PAIR_FN double dist2(double rx, double ry, double rz, double lx, double ly, double lz) {
    const double dx = rx - lx, dy = ry - ly, dz = rz - lz;
    return dx * dx + dy * dy + dz * dz;
}

// DFIRE's bin of a d2 <= 225 (src/dfire.rs:336-337) through the cell LUT and the exact steps (DESIGN.md "bin LUT")
LD_PAIR_FN uint32_t dfire_bin(double d2, const uint8_t *lut, const double *bin_step) {
    uint32_t bin = lut[(int)(d2 * 4.0)];
    bin += d2 >= bin_step[bin + 1] ? 1u : 0u;
    return bin;
}

// DNA constants, src/dna.rs:15-25
constexpr double kElecCutoff2 = 30.0 * 30.0;
constexpr double kVdwCutoff2 = 10.0 * 10.0;
constexpr double kElecMax = 1.0 * 4.0 / 332.0;
constexpr double kElecMin = -1.0 * 4.0 / 332.0;
constexpr double kVdwMax = 1.0;

LD_PAIR_FN double powi3(double x) { return x * x * x; }
LD_PAIR_FN double powi6(double x) {
    const double x2 = x * x;
    return x2 * (x2 * x2);
}

// src/dna.rs:481-491: the clamps are the reference's comparisons
LD_PAIR_FN double dna_elec(double q_rec, double q_lig, double d2) {
    double e = q_rec * q_lig / d2;
    if (e > kElecMax) e = kElecMax;
    if (e < kElecMin) e = kElecMin;
    return e;
}

// src/dna.rs:494-504
LD_PAIR_FN double dna_vdw(double eps_rec, double eps_lig, double r_rec, double r_lig, double d2) {
    const double vdw_energy = sqrt(eps_rec * eps_lig);
    const double vdw_radius = r_rec + r_lig;
    const double p6 = powi6(vdw_radius) / powi3(d2);
    double k = vdw_energy * (p6 * p6 - 2.0 * p6);
    if (k > kVdwMax) k = kVdwMax;
    return k;
}

}  // namespace decompose
}  // namespace ld
