// xlink.hpp -- launch interface of K3k, the cross-links of every pose: straight distances and shortest solvent paths on a
// lattice (kernels/xlink.hip; lightdock_hip.h, "Cross-links"): what the host side (xlink.cpp) and the
// kernels share, and the integer rule itself (the exact square root, the weights, a search box, a blocker's span of lattice
// nodes in a row), which is host code too so that a CPU build restates it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels/ccs.hpp"
#include "kernels/cluster.hpp"
#include "kernels/sasa.hpp"
#include "lightdock_hip.h"

namespace ld {

constexpr int kXlinkThreads = 512;
constexpr int kXlinkSlots = 512;            // 256 CUs x 2 resident workgroups (48 KiB of LDS each)
constexpr int kXlinkMaxLinks = 4096;
constexpr int kXlinkMinCell = 500, kXlinkMaxCell = 2000;  // thousandths
constexpr int kXlinkMaxReach = 6000;
constexpr int kXlinkMaxLength = 60000;
constexpr int kXlinkMaxSteps = 80;           // floor(M / h) at most: a box of 161 nodes an axis, 162 where h does not divide M
constexpr int kXlinkLdsWords = 12288;        // a box's blocked bits live in LDS up to 48 KiB (73^3 bits: the default's 71^3 and its rim)
constexpr int kXlinkMaxE = kSasaMaxRadius + kSasaMaxProbe;
constexpr uint32_t kXlinkNoPath = LD_XLINK_NO_PATH;
constexpr uint16_t kXlinkUnreached = 0xFFFF;

// --- the rule, on integers (thousandths) ------------------------------------------------------------------------------

// floor(sqrt(v)) for v < 2^52: the double root is at most one off, the integer steps settle it.
__host__ __device__ inline long long xlink_isqrt(long long v) {
    long long r = (long long)__builtin_sqrt((double)v);
    while (r * r > v) r--;
    while ((r + 1) * (r + 1) <= v) r++;
    return r;
}

// |a - b|^2 of two atoms' thousandths: each difference is within 2^31, the sum of three squares within 2^64.
__host__ __device__ inline unsigned long long xlink_square(const int a[3], const int b[3]) {
    unsigned long long s = 0;
    for (int k = 0; k < 3; k++) {
        const long long d = (long long)a[k] - (long long)b[k];
        s += (unsigned long long)(d * d);
    }
    return s;
}

// The search box of a source anchor at c: on every axis the nodes lo .. lo + n - 1 (times h) within M of c: 2 floor(M / h) + 1
// of them at most where h divides M, one more where it does not (c = 0.6 h, M = 1.6 h: the nodes -1 .. 2).  The field and
// the blocked bits of a box have a rim of one node all round, so a node's 26 neighbours are addressed without a test:
// node (i, j, k) of the box, each from 0, is word ((k + 1) py + (j + 1)) px + (i + 1).
struct XlinkBox {
    int lo[3], n[3];
    __host__ __device__ int px() const { return n[0] + 2; }
    __host__ __device__ int py() const { return n[1] + 2; }
    __host__ __device__ int pz() const { return n[2] + 2; }
    __host__ __device__ int padded() const { return px() * py() * pz(); }
    __host__ __device__ int index(int i, int j, int k) const { return ((k + 1) * py() + (j + 1)) * px() + (i + 1); }
};
__host__ __device__ inline XlinkBox xlink_box(const int c[3], int M, int h) {
    XlinkBox b;
    for (int k = 0; k < 3; k++) {
        b.lo[k] = ccs_ceil_div(c[k] - M, h);
        b.n[k] = ccs_floor_div(c[k] + M, h) - b.lo[k] + 1;
    }
    return b;
}
// The padded nodes of the largest box of a call.
inline size_t xlink_max_nodes(int M, int h) {
    const size_t side = 2 * (size_t)(M / h) + 3 + (M % h ? 1 : 0);
    return side * side * side;
}

// The nodes lo .. hi of the lattice row (., j h, k h) that the blocker (x, y, z, E) blocks: (i h - x)^2 + dy^2 + dz^2 < E^2,
// strictly, i.e. |i h - x| <= isqrt(E^2 - dy^2 - dz^2 - 1).  False when there is none.  E <= kXlinkMaxE: E^2 fits an int.
__host__ __device__ inline bool xlink_row_span(int x, int y, int z, int E, long long jh, long long kh, int h, int &lo, int &hi) {
    const long long dy = jh - y, dz = kh - z;
    if (dy >= E || dy <= -E || dz >= E || dz <= -E) return false;
    const long long v = (long long)E * E - dy * dy - dz * dz;
    if (v < 1) return false;
    const int w = (int)xlink_isqrt(v - 1);
    lo = ccs_ceil_div(x - w, h);
    hi = ccs_floor_div(x + w, h);
    return lo <= hi;
}

// --- the launches -----------------------------------------------------------------------------------------------------

struct XlinkDevice {
    int n_part = 0;                         // the blockers: the atoms that take part in the surface (SasaDevice's)
    const uint32_t *part_atom = nullptr;    // their complex atom indices
    const uint32_t *part_radius = nullptr;  // their radii R, thousandths
    int probe = 0, h = 0, reach = 0, M = 0;  // p, h, rho, M: thousandths
    int w2 = 0, w3 = 0;                     // isqrt(2 h^2), isqrt(3 h^2)
    int rmax = 0;                           // the rows an axis of a blocker touches at most: 2 (E_max - 1) / h + 1; n_part * rmax^2 <= INT_MAX
    int n_links = 0;                        // L, the row length of the outputs
    // the links grouped by source anchor: source s has the entries first[s] .. first[s + 1) - 1, entry e the other anchor
    // target[e] and the link number link[e] it answers
    int n_sources = 0;
    const uint32_t *source = nullptr;       // n_sources complex atom indices
    const uint32_t *first = nullptr;        // n_sources + 1
    const uint32_t *target = nullptr;       // L complex atom indices
    const uint32_t *link = nullptr;         // L link numbers
};

inline size_t xlink_align16(size_t bytes) { return (bytes + 15) / 16 * 16; }
inline bool xlink_bits_in_lds(int M, int h) { return (xlink_max_nodes(M, h) + 31) / 32 <= (size_t)kXlinkLdsWords; }
// A workspace slot: the culled blockers (int4 x, y, z, E), the 16-bit field of the padded box and, when they do not fit
// kXlinkLdsWords of LDS, the blocked bits of the padded box.
inline size_t xlink_field_offset(int n_part) { return xlink_align16((size_t)n_part * sizeof(int4)); }
inline size_t xlink_bits_offset(int n_part, int M, int h) { return xlink_field_offset(n_part) + xlink_align16(xlink_max_nodes(M, h) * sizeof(uint16_t)); }
inline size_t xlink_slot_bytes(int n_part, int M, int h) {
    return xlink_bits_offset(n_part, M, h) + (xlink_bits_in_lds(M, h) ? 0 : xlink_align16((xlink_max_nodes(M, h) + 31) / 32 * sizeof(uint32_t)));
}

// Reads `m` as ComplexDevice says and pose rows of 7 + m.anm_rec + m.anm_lig doubles, `stride` doubles apart.
// links: L x 2 complex atom indices; straight2: n x L.  overflow: one int, bit 0 set when a posed anchor is beyond +-1.0e6 A.
hipError_t launch_xlink_straight(const ComplexDevice &m, const double *poses, size_t stride, size_t n, const uint32_t *links, int n_links,
                                 unsigned long long *straight2, int *overflow, hipStream_t stream);

// `slots` workgroups, 1 .. kXlinkSlots, over the n x d.n_sources jobs (pose, source).  ws: slots x xlink_slot_bytes(d.n_part,
// d.M, d.h); path: n x d.n_links, every word written unless the pose overflows; overflow: one int, bit 0 set when a posed
// blocker or anchor is beyond +-1.0e6 A.
hipError_t launch_xlink_paths(const ComplexDevice &m, const XlinkDevice &d, const double *poses, size_t stride, size_t n, size_t slots,
                              void *ws, uint32_t *path, int *overflow, hipStream_t stream);

}  // namespace ld
