// complex_pose.hpp -- device code the analysis kernels share (kernels/cluster.hip, kernels/assess.hip, kernels/ranked.hip, kernels/sasa.hip, kernels/fcc.hip):
// the posing of one atom of a complex, the rounding to the thousandths "%8.3f" prints, the clustering's RMSD test, the
// 32-bit contact test on two atoms' thousandths, and the integer boxes with their exact distance test.
// Include from a .hip file only.
// Posing: receptor R_a + sum_m rec_ext[m] rec_mode[m][a]; ligand rotate(q, L_a + sum_m lig_ext[m] lig_mode[m][a]) + t,
// i.e. the ligand's modes in the ligand frame -- NOT the energy's convention (src/dfire.rs:282-302).  f64, qt.rs order,
// -ffp-contract=off.
#pragma once

#include "kernels/cluster.hpp"

namespace ld {

namespace {

struct P3 {
    double x, y, z;
};

// Complex atom `atom` (receptor atoms first, then ligand atoms) at the pose in `row`.
__device__ __forceinline__ P3 pose_atom(const ComplexDevice &m, const double *row, uint32_t atom) {
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
__device__ __forceinline__ double thousandths(double x) {
    const double p = x * 1000.0;
    const double e = fma(x, 1000.0, -p);
    const double f = floor(p);
    if (p - f == 0.5) {
        if (e > 0.0) return f + 1.0;
        if (e < 0.0) return f;
    }
    return rint(p);  // round half to even, as printf does on an exact tie
}

// round(rmsd, 4) <= cutoff with rmsd = sqrt(S / n) in A, S in thousandths^2.  Non-decreasing in S.
// Exactly: 400 S < n (2K + 1)^2, K the largest integer with K / 1e4 <= cutoff; only at equality does the rounding here decide.
__device__ __forceinline__ bool within_cutoff(double S, double n, double cutoff) {
    return rint(sqrt(S * 1e-6 / n) * 1e4) / 1e4 <= cutoff;
}

// --- the contact test on two atoms' thousandths (int4: x, y, z, unused), for cutoffs C <= 30000 -----------------------

constexpr uint32_t kAxisClamp = 32767;         // > 30000 >= C

// min(|d|, 32767) of a coordinate difference.  32767 > 30000 >= C: a clamped axis alone already exceeds the cutoff,
// so clamping never changes dx^2 + dy^2 + dz^2 <= C^2, and the sum of three squares stays below 3 * 2^30 < 2^32:
// 24-bit multiplies and one 32-bit compare, no 64-bit arithmetic.
__device__ __forceinline__ uint32_t clamped_abs(int d) { return min((uint32_t)abs(d), kAxisClamp); }

__device__ __forceinline__ uint32_t square_sum(uint32_t x, uint32_t y, uint32_t z) {
    return __umul24(x, x) + __umul24(y, y) + __umul24(z, z);
}

__device__ __forceinline__ bool in_contact(const int4 &a, const int4 &b, uint32_t C2) {
    return square_sum(clamped_abs(a.x - b.x), clamped_abs(a.y - b.y), clamped_abs(a.z - b.z)) <= C2;
}

// --- residue and group boxes on the thousandths (kernels/cluster.hip, kernels/fcc.hip) ---------------------------------

// Box b of a pose is box[k * n_boxes + b], k = min x, y, z, max x, y, z: consecutive lanes read consecutive words.
// b: residues (receptor, then ligand), receptor groups, ligand groups.
struct Box {
    int lo[3], hi[3];
};

__device__ __forceinline__ Box load_box(const int *box, int n_boxes, int b) {
    Box v;
    for (int k = 0; k < 3; k++) {
        v.lo[k] = box[k * n_boxes + b];
        v.hi[k] = box[(3 + k) * n_boxes + b];
    }
    return v;
}

__device__ __forceinline__ void store_box(int *box, int n_boxes, int b, const Box &v) {
    for (int k = 0; k < 3; k++) {
        box[k * n_boxes + b] = v.lo[k];
        box[(3 + k) * n_boxes + b] = v.hi[k];
    }
}

// The gap between two intervals on one axis (0 when they overlap), clamped like a difference.
__device__ __forceinline__ uint32_t clamped_gap(int lo_a, int hi_a, int lo_b, int hi_b) {
    return min((uint32_t)max(max(lo_a - hi_b, lo_b - hi_a), 0), kAxisClamp);
}

// Exact: every atom pair of the two boxes is at least the gap apart on each axis, so a box distance above C (which an
// axis gap above C implies) leaves no pair within C.  Nothing is padded.
__device__ __forceinline__ bool boxes_within(const Box &a, const Box &b, uint32_t C2) {
    return square_sum(clamped_gap(a.lo[0], a.hi[0], b.lo[0], b.hi[0]), clamped_gap(a.lo[1], a.hi[1], b.lo[1], b.hi[1]),
                      clamped_gap(a.lo[2], a.hi[2], b.lo[2], b.hi[2])) <= C2;
}

}  // namespace

}  // namespace ld
