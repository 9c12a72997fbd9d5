// complex_rule.hpp -- the rule every analysis kernel starts with, host code too so that a CPU build restates it: the
// posing of one atom of a complex, the rounding to the thousandths "%8.3f" prints, and the bound and clamp on the result.
// kernels/complex_pose.hpp includes it for the kernels; ccs.cpp rounds the rigid receptor's atoms with it; the sanitizer
// build's stubs (tests/asan/hip_stub_*.cpp) pose with it in place of the kernels.
// Posing: receptor R_a + sum_m rec_ext[m] rec_mode[m][a]; ligand rotate(q, L_a + sum_m lig_ext[m] lig_mode[m][a]) + t,
// i.e. the ligand's modes in the ligand frame -- NOT the energy's convention (src/dfire.rs:282-302).  f64, qt.rs order,
// -ffp-contract=off.
#pragma once

#include <cmath>

#include "kernels/cluster.hpp"

namespace ld {

// thousandths: +-1.0e6 A.  Within it the difference of two coordinates fits an int32, and so does a projection of the
// collision cross-section (|a| < 1.74e9, kernels/ccs.hpp).
constexpr int kComplexCoordBound = 1000000000;

struct P3 {
    double x, y, z;
};

// Complex atom `atom` (receptor atoms first, then ligand atoms) at the pose in `row`.
__host__ __device__ __forceinline__ P3 pose_atom(const ComplexDevice &m, const double *row, uint32_t atom) {
    if ((int)atom < m.n_rec) {
        const double *r = m.rec_xyz + 3 * (size_t)atom;
        P3 p{r[0], r[1], r[2]};
        for (int k = 0; k < m.anm_rec; k++) {
            const double c = row[7 + k];
            const double *v = m.rec_modes + ((size_t)k * m.n_rec + atom) * 3;
            p.x += v[0] * c;
            p.y += v[1] * c;
            p.z += v[2] * c;
        }
        return p;
    }
    const uint32_t a = atom - (uint32_t)m.n_rec;
    const double *l = m.lig_xyz + 3 * (size_t)a;
    double vx = l[0], vy = l[1], vz = l[2];
    for (int k = 0; k < m.anm_lig; k++) {  // in the ligand frame, before the rotation
        const double c = row[7 + m.anm_rec + k];
        const double *v = m.lig_modes + ((size_t)k * m.n_lig + a) * 3;
        vx += v[0] * c;
        vy += v[1] * c;
        vz += v[2] * c;
    }
    const double qw = row[3], qx = row[4], qy = row[5], qz = row[6];
    // q * (0, v), src/qt.rs:174-185 with other.w = 0
    const double aw = qw * 0.0 - qx * vx - qy * vy - qz * vz;
    const double ax = qw * vx + qx * 0.0 + qy * vz - qz * vy;
    const double ay = qw * vy - qx * vz + qy * 0.0 + qz * vx;
    const double az = qw * vz + qx * vy - qy * vx + qz * 0.0;
    // q^-1 = conjugate / norm2, src/qt.rs:48-50
    const double n2 = qw * qw + qx * qx + qy * qy + qz * qz;
    const double bw = qw / n2, bx = -qx / n2, by = -qy / n2, bz = -qz / n2;
    // (q v) * q^-1, vector part
    const double rx = aw * bx + ax * bw + ay * bz - az * by;
    const double ry = aw * by - ax * bz + ay * bw + az * bx;
    const double rz = aw * bz + ax * by - ay * bx + az * bw;
    return P3{rx + row[0], ry + row[1], rz + row[2]};
}

// The integer c with "%.3f" of x == c / 1000 (exact: p + e is x * 1000 to the last bit; for |p| < 2^52
// only an exact .5 in p can round differently from the exact product, and the sign of e settles it).
__host__ __device__ __forceinline__ double thousandths(double x) {
    const double p = x * 1000.0;
    const double e = fma(x, 1000.0, -p);
    const double f = floor(p);
    if (p - f == 0.5) {
        if (e > 0.0) return f + 1.0;
        if (e < 0.0) return f;
    }
    return rint(p);  // round half to even, as printf does on an exact tie
}

// v: the thousandths of complex atom `atom` at the pose in `row`, each axis clamped to +-bound so that nothing later can
// wrap (a NaN clamps to +bound).  False when an axis was beyond the bound or NaN: the caller fails the call.
__host__ __device__ __forceinline__ bool posed_thousandths(const ComplexDevice &m, const double *row, uint32_t atom, int bound,
                                                           int v[3]) {
    const P3 p = pose_atom(m, row, atom);
    const double c[3] = {thousandths(p.x), thousandths(p.y), thousandths(p.z)};
    bool ok = true;
    for (int k = 0; k < 3; k++) {
        if (!(fabs(c[k]) <= (double)bound)) ok = false;
        v[k] = (int)fmax(-(double)bound, fmin((double)bound, c[k]));
    }
    return ok;
}

}  // namespace ld
