// ccs.hpp -- launch interface of K3j, the collision cross-section of every pose by the projection approximation
// (kernels/ccs.hip; lightdock_hip.h, "Collision cross-section"): what the host side (ccs.cpp) and the
// kernels share, and the integer rule itself (frames, projection, floor division, the exact square root, a row's span of
// lattice columns), which is host code too so that a CPU build restates it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels/cluster.hpp"
#include "kernels/sasa.hpp"
#include "lightdock_hip.h"

namespace ld {

constexpr int kCcsViews = LD_CCS_VIEWS;
constexpr int kCcsThreads = 512;
constexpr int kCcsSlots = kContactSlots;
constexpr int kCcsBitmapWords = 12288;       // a workgroup's bitmap: 48 KiB of LDS, 393 216 lattice points a piece
constexpr int kCcsMinCell = 100, kCcsMaxCell = 2000;  // thousandths
constexpr int kCcsMaxE = kSasaMaxRadius + kSasaMaxProbe;
constexpr long long kCcsMaxBox = 1ll << 28;  // lattice points of a view's box: a count fits 32 bits
constexpr size_t kCcsRigidBytes = size_t(64) << 20;  // the rigid receptor's 64 bitmaps at most; beyond it every pose rasterises it

// --- the rule, on integers (thousandths) ------------------------------------------------------------------------------

// 64 x 6: rint(2^20 * e1) then rint(2^20 * e2) of every view (tools/gen_ccs_frames.py)
inline constexpr int32_t kCcsFrames[kCcsViews][6] = {
#include "kernels/ccs_frames.inc"
};

// One in-plane coordinate of the atom at (x, y, z): (F . c + 2^19) >> 20, the dot product in 64 bits, the shift arithmetic.
__host__ __device__ inline int ccs_project(const int32_t *F, int x, int y, int z) {
    return (int)(((long long)F[0] * x + (long long)F[1] * y + (long long)F[2] * z + (1ll << 19)) >> 20);
}

// floor(x / h) and ceil(x / h) for h > 0 and any sign of x: a quotient that truncates is put right.
__host__ __device__ inline int ccs_floor_div(int x, int h) {
    const int q = x / h;
    return x % h < 0 ? q - 1 : q;
}
__host__ __device__ inline int ccs_ceil_div(int x, int h) {
    const int q = x / h;
    return x % h > 0 ? q + 1 : q;
}

// floor(sqrt(v)) for 0 <= v <= kCcsMaxE^2 < 2^24: the float root is at most one off, the integer steps settle it.
__host__ __device__ inline int ccs_isqrt(int v) {
    int r = (int)__builtin_sqrtf((float)v);
    while (r * r > v) r--;
    while ((r + 1) * (r + 1) <= v) r++;
    return r;
}

// The lattice columns [lo, hi] of row j that the disc of radius E about (a, b) covers: (i h - a)^2 + (j h - b)^2 <= E^2.
// False when the row misses the disc or no column lies inside.  |a|, |b| < 1.74e9 and |j h - b| <= E + h for the rows a
// caller asks about, so every term fits an int32 but j * h - b, which is formed in 64 bits.
__host__ __device__ inline bool ccs_row_span(int a, int b, int E, int j, int h, int &lo, int &hi) {
    const long long dy = (long long)j * h - b;
    if (dy > E || dy < -E) return false;
    const int w = ccs_isqrt(E * E - (int)dy * (int)dy);
    lo = ccs_ceil_div(a - w, h);
    hi = ccs_floor_div(a + w, h);
    return lo <= hi;
}

// The bits lo_bit .. hi_bit of a word, 0 <= lo_bit <= hi_bit <= 31.
__host__ __device__ inline uint32_t ccs_mask(int lo_bit, int hi_bit) { return (0xffffffffu << lo_bit) & (0xffffffffu >> (31 - hi_bit)); }

// A view's box of lattice points: columns i0 .. i1 and rows j0 .. j1 that [lo_a, hi_a] x [lo_b, hi_b] touches (the
// extremes of a - E, a + E, b - E, b + E over the atoms).  A bitmap row holds the 32-column words wc0 .. wc1 (word i >> 5,
// bit i & 31, the shift arithmetic: the words of every bitmap line up whatever box they were made for).
struct CcsBox {
    int i0, i1, j0, j1;
    __host__ __device__ long long columns() const { return (long long)i1 - i0 + 1; }
    __host__ __device__ long long rows() const { return (long long)j1 - j0 + 1; }
    __host__ __device__ int wc0() const { return i0 >> 5; }
    __host__ __device__ int wc1() const { return i1 >> 5; }
};
__host__ __device__ inline CcsBox ccs_box(int lo_a, int hi_a, int lo_b, int hi_b, int h) {
    return CcsBox{ccs_ceil_div(lo_a, h), ccs_floor_div(hi_a, h), ccs_ceil_div(lo_b, h), ccs_floor_div(hi_b, h)};
}

// --- the launches -----------------------------------------------------------------------------------------------------

// One view of the rigid receptor: the extremes of its atoms' discs, and where its bitmap lies in rec_bits: rows j0 ..
// j0 + rows - 1 of `pitch` words each, the first of them word column wc0.
struct CcsRecView {
    int lo_a, hi_a, lo_b, hi_b;
    int wc0, j0, pitch, rows;
    unsigned long long offset;  // in words
};

struct CcsDevice {
    int first = 0, count = 0;  // the atoms posed for every pose: part_atom[first .. first + count)
    int h = 0;                 // the lattice step, thousandths
    int probe = 0;             // p, thousandths
    int rmax = 0;              // the rows an atom touches at most: 2 e_max / h + 1; count * rmax <= INT_MAX
    const uint32_t *part_atom = nullptr;    // complex atom indices of the atoms that take part (SasaDevice's)
    const uint32_t *part_radius = nullptr;  // their radii R, thousandths
    // the rigid-receptor form, null without it: the receptor's atoms are not among [first, first + count)
    const CcsRecView *rec_views = nullptr;  // kCcsViews
    const uint32_t *rec_bits = nullptr;
};

// A workspace slot: the posed atoms (x, y, z, E) and their projection in the view at hand (a, b, E, first row).
inline size_t ccs_slot_bytes(int count) { return (size_t)count * 2 * sizeof(int4); }

// The rigid receptor's bitmaps, once a call: view v of atoms (x, y, z, E) into rec_bits as views[v] lays it out; rec_bits
// ZEROED by the caller.
hipError_t launch_ccs_receptor(const int4 *atoms, int n_atoms, int h, int rmax, const CcsRecView *views, uint32_t *rec_bits,
                               hipStream_t stream);

// `slots` workgroups, 1 .. kCcsSlots.  Reads `m` as ComplexDevice says and pose rows of 7 + m.anm_rec + m.anm_lig doubles,
// `stride` doubles apart.  ws: slots x ccs_slot_bytes(d.count); counts: n x kCcsViews; sums: n; overflow: one int, bit 0 set
// when a posed coordinate is beyond +-1.0e6 A, bit 1 when a view's box holds more than kCcsMaxBox lattice points (the
// counts and the sum of such a pose are not written).
hipError_t launch_complex_ccs(const ComplexDevice &m, const CcsDevice &d, const double *poses, size_t stride, size_t n, size_t slots,
                              void *ws, uint32_t *counts, unsigned long long *sums, int *overflow, hipStream_t stream);

}  // namespace ld
