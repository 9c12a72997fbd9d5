// complex_pose.hpp -- device code the analysis kernels share (kernels/cluster.hip, kernels/assess.hip, kernels/ranked.hip, kernels/sasa.hip,
// kernels/fcc.hip, kernels/saxs.hip, kernels/emfit.hip, kernels/ccs.hip): the clustering's RMSD test, the 32-bit contact test on two atoms'
// thousandths, and the integer boxes with their exact distance test.  The posing of one atom, the rounding to the thousandths "%8.3f"
// prints and the coordinate bound are host code too: kernels/complex_rule.hpp, included here.
// Include from a .hip file only.
#pragma once

#include "kernels/complex_rule.hpp"

namespace ld {

namespace {

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
