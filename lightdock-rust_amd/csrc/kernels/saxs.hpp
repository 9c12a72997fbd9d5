// saxs.hpp -- launch interface of K3h, the SAXS profile of every pose (kernels/saxs.hip; lightdock_hip.h,
// "Small-angle scattering"): what the host side (saxs.cpp) and the kernels share, and the integer rule itself (classes,
// pair classes, the clamped difference, the bin of a squared distance), which is host code too so that a CPU build
// restates it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels/cluster.hpp"
#include "lightdock_hip.h"

namespace ld {

constexpr int kSaxsClasses = LD_SAXS_CLASSES;
constexpr int kSaxsPairClasses = LD_SAXS_PAIR_CLASSES;
constexpr int kSaxsNoPart = 255;             // the class of an atom that takes no part
constexpr int kSaxsMaxAtoms = 65536;         // taking part: a bin count, at most n (n - 1) / 2, fits 32 bits
constexpr int kSaxsMaxBins = 1024;
constexpr int kSaxsMinWidth = 100, kSaxsMaxWidth = 2000;  // thousandths
constexpr int kSaxsMaxQ = 1024;
constexpr int kSaxsThreads = 512;            // of the histogram kernel: two halves, each half a b-tile's half
constexpr int kSaxsTile = 256;               // atoms of a tile: an a-atom a lane of a half
constexpr int kSaxsPoseThreads = 256;
constexpr int kSaxsDebyeThreads = 256;
constexpr int kSaxsTargetGroups = 2048;      // workgroups the histogram launch aims at: 256 CUs x up to 3 resident, and a tail
constexpr uint32_t kSaxsAxisClamp = (1u << 22) - 1;  // > 1024 x 2000: a clamped pair is beyond the last bin anyway
// The kernel's f32 estimate of d / w: the differences are exact in f32 below 2^24, the sum of three squares takes three
// roundings (relative error 3 u, u = 2^-24), v_sqrt_f32 halves that and adds its 1 ulp (2 u), 1 / w and the product add
// u each: 5.5 u in all, so below 2^-10 / 5.5 u = 2978 bins the estimate is within 2^-10 of d / w.  Its floor is the bin
// unless the estimate lies within kSaxsEdge of an integer; then, and only then, saxs_bin decides on d^2 in 64 bits.
// Beyond 2978 the floor may be one off, which no call can see: bins <= 1024, and every such pair is an overflow.
constexpr float kSaxsEdge = 1.0f / 1024.0f;

// --- the rule, on integers (thousandths) ------------------------------------------------------------------------------

// Pair class of classes e, f (either order), 0 .. 20: with e <= f, 6 e - e (e - 1) / 2 + (f - e).
__host__ __device__ inline uint32_t saxs_pair_class(uint32_t e, uint32_t f) {
    const uint32_t lo = e < f ? e : f, hi = e < f ? f : e;
    return 6 * lo - lo * (lo - 1) / 2 + (hi - lo);
}

// The six pair classes of class e as 5-bit fields, field f = saxs_pair_class(e, f).
__host__ __device__ inline uint32_t saxs_pair_fields(uint32_t e) {
    uint32_t packed = 0;
    for (uint32_t f = 0; f < (uint32_t)kSaxsClasses; f++) packed |= saxs_pair_class(e, f) << (5 * f);
    return packed;
}

// min(|d|, 2^22 - 1) of a coordinate difference.
__host__ __device__ inline uint32_t saxs_axis(int d) {
    const uint32_t a = d < 0 ? 0u - (uint32_t)d : (uint32_t)d;
    return a < kSaxsAxisClamp ? a : kSaxsAxisClamp;
}

// d^2 of three clamped differences: below 3 x 2^44, exact.
__host__ __device__ inline unsigned long long saxs_d2(uint32_t x, uint32_t y, uint32_t z) {
    return (unsigned long long)x * x + (unsigned long long)y * y + (unsigned long long)z * z;
}

// The bin of d2 at width w: the largest k with (k w)^2 <= d2, from an estimate within one of it.
__host__ __device__ inline uint32_t saxs_bin(unsigned long long d2, uint32_t w, uint32_t k) {
    const unsigned long long kw = (unsigned long long)k * w, lo = kw * kw, hi = lo + (2 * kw + w) * w;  // ((k + 1) w)^2
    return d2 < lo ? k - 1 : d2 >= hi ? k + 1 : k;
}

// The class of an ATOM / HETATM record, kSaxsNoPart for one that takes no part: a residue named MMB or an element that is
// none of H (D), C, N, O, P, S.  The element by the surface's rule (sasa_radius).  `line` has 54 columns at least.
uint8_t saxs_class(const char *line, size_t len);

struct SaxsDevice {
    int n_part = 0, n_part_rec = 0;       // atoms that take part, the receptor's first
    const uint32_t *part_atom = nullptr;  // n_part complex atom indices, ascending
    const uint8_t *part_class = nullptr;  // n_part classes, 0 .. 5
};

struct SaxsHistogram {
    int n_atoms = 0;       // atoms of a row of `atoms`
    int first_b = 0;       // a pair (a < b) counts when b >= first_b: the receptor's own pairs are left to the base row
    uint32_t width = 0;    // w
    int bins = 0;
    int splits = 0;        // workgroups a pose
    const int4 *atoms = nullptr;  // poses x atom_stride (x, y, z, class)
    size_t atom_stride = 0;
    uint32_t *counts = nullptr;   // poses x 21 x bins, initialised by the caller
    int *overflow = nullptr;      // one int, set when a pair lies beyond the last bin or a coordinate beyond the bound
};

// Tile pairs (ta <= tb) that hold a pair with b >= first_b, and the workgroups a pose that `poses` poses are split into.
inline int saxs_tiles(int n_atoms) { return (n_atoms + kSaxsTile - 1) / kSaxsTile; }
inline long long saxs_tile_pairs(int n_atoms, int first_b) {
    const long long nt = saxs_tiles(n_atoms), t0 = first_b / kSaxsTile;
    return nt * (nt + 1) / 2 - t0 * (t0 + 1) / 2;
}
inline int saxs_splits(int n_atoms, int first_b, size_t poses) {
    const long long pairs = saxs_tile_pairs(n_atoms, first_b), want = ((long long)kSaxsTargetGroups + (long long)poses - 1) / (long long)poses;
    return (int)(want < 1 ? 1 : want > pairs ? (pairs < 1 ? 1 : pairs) : want);
}
// The words of a row in LDS, and the histogram kernel's spare word behind them.
inline size_t saxs_histogram_lds_bytes(int bins) { return ((size_t)kSaxsPairClasses * bins + 1) * sizeof(uint32_t); }

// Every launch reads `m` as ComplexDevice says and pose rows of 7 + m.anm_rec + m.anm_lig doubles, `stride` doubles apart.

// Atoms first .. first + count of d's list at each of n poses -> out[pose * out_stride + (a - first)] as (x, y, z, class);
// overflow: set when a coordinate is beyond +-1.0e6 A (the stored value is clamped).
hipError_t launch_saxs_pose(const ComplexDevice &m, const SaxsDevice &d, const double *poses, size_t stride, size_t n, int first,
                            int count, int4 *out, size_t out_stride, int *overflow, hipStream_t stream);
// rows[p][i] = base[i] (or 0 with base == nullptr), i < row_words.
hipError_t launch_saxs_rows(const uint32_t *base, uint32_t *rows, size_t n, size_t row_words, hipStream_t stream);
// h.splits workgroups a pose add the pairs of their tile-pair range to the pose's row.
hipError_t launch_saxs_histogram(const SaxsHistogram &h, size_t n, hipStream_t stream);

struct SaxsDebye {
    int bins = 0, n_q = 0;
    const uint32_t *counts = nullptr;  // poses x 21 x bins
    const double *sinc_t = nullptr;    // bins x n_q: s(q_j r_k) at [k * n_q + j]
    const double *self = nullptr;      // n_q: S_j
    const double *cross = nullptr;     // n_q x 21: F_{j,c}
    double *intensity = nullptr;       // poses x n_q
};
// One workgroup a pose.
hipError_t launch_saxs_debye(const SaxsDebye &d, size_t n, hipStream_t stream);

}  // namespace ld
