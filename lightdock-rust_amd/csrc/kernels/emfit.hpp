// emfit.hpp -- launch interface of K3i, the fit of every pose to a density map (kernels/emfit.hip; DESIGN §5 K3i;
// lightdock_hip.h, "Density fit"): what the host side (emfit.cpp) and the kernels share, and the integer rule itself (the
// weight of a class, a voxel's centre, the term an atom adds to a voxel, the cell test of `outside`), which is host code too
// so that a CPU build restates the kernels from it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels/cluster.hpp"
#include "kernels/saxs.hpp"
#include "lightdock_hip.h"

namespace ld {

constexpr int kEmfitMaxAxis = 1024;                 // voxels an axis
constexpr size_t kEmfitMaxVoxels = (size_t)1 << 24;
constexpr int kEmfitMinStep = 200, kEmfitMaxStep = 20000;      // thousandths
constexpr int kEmfitOriginBound = 1000000000;
constexpr int kEmfitMinSigma = 300, kEmfitMaxSigma = 15000;    // thousandths
constexpr int kEmfitMaxTable = 4096;                // entries of the kernel table
constexpr int kEmfitMaxAtoms = kSaxsMaxAtoms;       // taking part: 65536 x 16 x 255 < 2^32, a voxel cannot wrap
constexpr int kEmfitReachVoxels = 16;               // a support wider than this many voxels of the finest axis is refused
constexpr uint32_t kEmfitVoxelLimit = 1u << 24;     // a simulated voxel at or above it sets the overflow word
constexpr unsigned long long kEmfitSumLimit = 1ull << 40;  // so does S_s at or above this
constexpr int kEmfitBrick = 16;                     // a brick is 16 x 16 voxels on x and y ...
constexpr int kEmfitDepth = 4;                      // ... and this many on z
constexpr int kEmfitThreads = kEmfitBrick * kEmfitBrick;  // of the brick kernel: a thread a column of kEmfitDepth voxels along z
constexpr int kEmfitPoseThreads = 256;
constexpr int kEmfitListThreads = 64;
constexpr int kEmfitMaxGroups = 2048;               // workgroups of the brick launch: 256 CUs x 8 resident

// --- the rule, on integers (thousandths) ------------------------------------------------------------------------------

// The atomic number of class 0 .. 5: H, C, N, O, P, S.
__host__ __device__ inline uint32_t emfit_weight(uint32_t cls) {
    return cls == 0 ? 1u : cls == 1 ? 6u : cls == 2 ? 7u : cls == 3 ? 8u : cls == 4 ? 15u : 16u;
}

// What the kernels know of a map.  A voxel's centre on axis k is origin[k] + i step[k]: below 2^31 (|origin| <= 10^9,
// 1023 x 20000 beyond it), and its difference from a coordinate within +-10^9 fits an int32 too.
struct EmfitMap {
    int n[3] = {0, 0, 0};
    int origin[3] = {0, 0, 0};
    int step[3] = {0, 0, 0};
    const uint16_t *E = nullptr;  // the quantised voxels, x fastest
    __host__ __device__ size_t voxels() const { return (size_t)n[0] * n[1] * n[2]; }
    __host__ __device__ static int brick_size(int k) { return k == 2 ? kEmfitDepth : kEmfitBrick; }
    __host__ __device__ int bricks(int k) const { return (n[k] + brick_size(k) - 1) / brick_size(k); }
    __host__ __device__ size_t n_bricks() const { return (size_t)bricks(0) * bricks(1) * bricks(2); }
};

// The kernel table of a sigma: K[d2 >> shift] for d2 < limit = length << shift, nothing beyond.  limit < 2^32 for every
// sigma the rule admits (at 15000: 2676 << 20), so reach = isqrt(limit - 1) < 2^16: an axis difference above reach alone
// puts d2 at or beyond the limit, and the squares of differences up to reach fit 32 bits each.
struct EmfitTable {
    uint32_t shift = 0, length = 0, limit = 0, reach = 0;
    const uint8_t *K = nullptr;  // length entries, each <= 255
};

__host__ __device__ inline uint32_t emfit_abs(int d) { return d < 0 ? 0u - (uint32_t)d : (uint32_t)d; }

// The table index of the squared distance of three axis differences, or -1 at or beyond the limit.  Exact: an axis
// beyond reach decides alone; otherwise y^2 + z^2 is taken in 64 bits and x^2 joins it only below the limit.
__host__ __device__ inline int emfit_index(int dx, int dy, int dz, uint32_t shift, uint32_t limit, uint32_t reach) {
    const uint32_t ax = emfit_abs(dx), ay = emfit_abs(dy), az = emfit_abs(dz);
    if (ax > reach || ay > reach || az > reach) return -1;
    const unsigned long long d2 = (unsigned long long)ax * ax + (unsigned long long)ay * ay + (unsigned long long)az * az;
    return d2 < limit ? (int)((uint32_t)d2 >> shift) : -1;
}

// An atom at coordinate x lies in no voxel's cell on an axis of n voxels from origin at step h:
// 2 (x - X[0]) < -h or 2 (x - X[n - 1]) >= h.
__host__ __device__ inline bool emfit_axis_outside(int x, int origin, int h, int n) {
    const long long lo = 2ll * ((long long)x - origin), hi = 2ll * ((long long)x - ((long long)origin + (long long)(n - 1) * h));
    return lo < -(long long)h || hi >= (long long)h;
}

// floor(a / b), b > 0.
__host__ __device__ inline long long emfit_floor_div(long long a, long long b) {
    const long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// The voxel indices lo .. hi of an axis whose centres lie within `reach` of the interval [a_lo, a_hi], clipped to the
// grid; lo > hi when there is none.
__host__ __device__ inline void emfit_axis_range(int a_lo, int a_hi, uint32_t reach, int origin, int h, int n, int *lo, int *hi) {
    const long long first = -emfit_floor_div(-((long long)a_lo - (long long)reach - origin), h);  // ceil
    const long long last = emfit_floor_div((long long)a_hi + (long long)reach - origin, h);
    *lo = (int)(first < 0 ? 0 : first > n ? n : first);
    *hi = (int)(last > n - 1 ? n - 1 : last < -1 ? -1 : last);
}

// --- launches -----------------------------------------------------------------------------------------------------------

// A pose's box: min x, y, z, max x, y, z of the atoms posed for it (INT_MAX / INT_MIN without one).
struct EmfitBox {
    int lo[3], hi[3];
};

// rows[p] = *from (or zeros with from == nullptr), boxes[p] = empty, p < n.
hipError_t launch_emfit_init(ld_density_sums *rows, EmfitBox *boxes, const ld_density_sums *from, size_t n, hipStream_t stream);
// grid[p][v] = base[v] (or 0 with base == nullptr), v < voxels.
hipError_t launch_emfit_fill(uint32_t *grid, const uint32_t *base, size_t n, size_t voxels, hipStream_t stream);
// Atoms first .. first + count of d's list at each of n poses -> out[pose * out_stride + (a - first)] as (x, y, z, weight);
// the pose's box grows by them, rows[pose].outside counts those in no voxel's cell; overflow: set when a coordinate is
// beyond +-1.0e6 A (the stored value is clamped).
hipError_t launch_emfit_pose(const ComplexDevice &m, const SaxsDevice &d, const EmfitMap &map, const double *poses, size_t stride, size_t n,
                             int first, int count, int4 *out, size_t out_stride, EmfitBox *boxes, ld_density_sums *rows, int *overflow,
                             hipStream_t stream);
// The bricks the supports of each pose's box can reach, appended to items as (pose, brick) from *n_items on.  The caller
// zeroes *n_items; items holds n x map.n_bricks() entries.
hipError_t launch_emfit_list(const EmfitMap &map, uint32_t reach, const EmfitBox *boxes, size_t n, uint2 *items, uint32_t *n_items,
                             hipStream_t stream);

struct EmfitBricks {
    EmfitMap map;
    EmfitTable table;
    int n_atoms = 0;                  // atoms of a row of `atoms`
    const int4 *atoms = nullptr;      // poses x atom_stride (x, y, z, weight)
    size_t atom_stride = 0;
    const uint2 *items = nullptr;     // (pose, brick)
    const uint32_t *n_items = nullptr;
    const uint32_t *base = nullptr;   // voxels every brick starts from, or nullptr for zeros
    const unsigned long long *base_sums = nullptr;  // bricks x 4 (s, ss, se, in) of `base`: taken off a visited brick's sums
    unsigned long long *brick_sums = nullptr;       // bricks x 4, written for every visited brick, or nullptr
    ld_density_sums *rows = nullptr;  // a row a pose, initialised by the caller
    uint32_t *grid = nullptr;         // poses x voxels, the visited bricks' voxels, or nullptr
    int *overflow = nullptr;          // set when a voxel reaches kEmfitVoxelLimit
};
// `groups` workgroups share the items, a brick at a time.
hipError_t launch_emfit_bricks(const EmfitBricks &b, size_t groups, hipStream_t stream);

}  // namespace ld
