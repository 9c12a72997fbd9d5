// sasa.hip -- K3f: the solvent-accessible surface of every pose and what the interface buries of it (gfx950; DESIGN §5
// K3f; lightdock_hip.h, "Solvent-accessible surface").  The kernel and its launcher (kernels/sasa.hpp); the host side is
// complex.cpp.  Shrake-Rupley on the thousandths "%8.3f" prints, all integers.
//   complex_sasa: one workgroup a pose at a time (a launch has at most kSasaSlots workgroups, each with a workspace slot it
//   reuses for pose blockIdx, blockIdx + gridDim, ...):
//     1. every atom that takes part is posed once (complex_rule.hpp), rounded and kept as int4 (x, y, z, E) in the slot;
//        the same pass folds it into the int32 box of its molecule in LDS;
//     2. a cell grid PER MOLECULE over that molecule's own box: the edge is the smallest multiple of 2 E_max + 2 at which
//        the grid has at most kSasaCells cells, so a huge extent coarsens the grid and never overflows the LDS offsets.
//        Count, exclusive scan, scatter: the atoms of both molecules ordered by cell in the slot, s_off[c] .. s_off[c + 1]
//        the atoms of cell c (the receptor's cells, then the ligand's);
//     3. a wave an atom, lane = point, two points a lane.  The cells an atom's reach E_a + E_max + 1 touches (three an
//        axis at most) are walked 64 atoms at a time; those with |c_a - c_b|^2 < (E_a + E_b + 1)^2 are compacted by ballot
//        into the wave's LDS list as (c_b - c_a, E_b^2), and whenever the next 64 might not fit, the points still exposed are
//        tested against the list and the list starts again: no list length truncates.  The own grid gives the free mask;
//        the other molecule's grid is walked only when the reach meets its box, over the points still exposed.  Counts are
//        popcounts of ballots; E_a^2 x count adds up per wave and meets the pose's four sums with one 64-bit integer
//        atomic a wave and sum.
// Integer sums are order-free and a burial is an OR over neighbours, so a pose's results are the same bits whatever the
// batch, its place in it, the slot count or the order of atoms inside a cell.
#include "kernels/sasa.hpp"

#include <climits>

#include "kernels/complex_pose.hpp"

namespace ld {

namespace {

constexpr int kWaves = kSasaThreads / 64;
constexpr int kScanRun = 2 * kSasaCells / kSasaThreads;  // offsets a thread scans
static_assert(kScanRun * kSasaThreads == 2 * kSasaCells, "the scan deals the offsets evenly");
static_assert(kSasaListCap >= 128, "a list takes 64 neighbours more before it is drained");
static_assert(2 * (kSasaMaxRadius + kSasaMaxProbe) + kSasaSlack < (int)kAxisClamp, "the clamped 32-bit neighbour test");

__device__ const int d_directions[kSasaPoints][3] = {
#include "kernels/sasa_directions.inc"
};

struct Grid {
    int lo[3];
    int n[3];
    uint32_t h;
};

// The grid of a box: the smallest multiple of h0 as the edge at which the cells are at most kSasaCells.  Uniform.
__device__ __forceinline__ Grid make_grid(const int *box, uint32_t h0) {
    Grid g;
    uint32_t ext[3];
    for (int k = 0; k < 3; k++) {
        g.lo[k] = __builtin_amdgcn_readfirstlane(box[k]);
        ext[k] = (uint32_t)__builtin_amdgcn_readfirstlane(box[3 + k]) - (uint32_t)g.lo[k];
    }
    uint32_t lo = 1, hi = 0x7fffffffu / h0;  // at hi an edge is beyond every extent: one cell
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2, h = mid * h0;
        const unsigned long long cells = (unsigned long long)(ext[0] / h + 1) * (ext[1] / h + 1) * (ext[2] / h + 1);
        if (cells <= (unsigned long long)kSasaCells) hi = mid;
        else lo = mid + 1;
    }
    g.h = lo * h0;
    for (int k = 0; k < 3; k++) g.n[k] = (int)(ext[k] / g.h) + 1;
    return g;
}

__device__ __forceinline__ int cell_of(const Grid &g, const int4 &v) {
    const uint32_t cx = ((uint32_t)v.x - (uint32_t)g.lo[0]) / g.h, cy = ((uint32_t)v.y - (uint32_t)g.lo[1]) / g.h,
                   cz = ((uint32_t)v.z - (uint32_t)g.lo[2]) / g.h;
    return (int)((cx * (uint32_t)g.n[1] + cy) * (uint32_t)g.n[2] + cz);
}

// The cells [c0, c1] of one axis that [v - reach, v + reach] touches; c1 < c0 when none.
__device__ __forceinline__ void cell_range(int v, int reach, int lo, uint32_t h, int n, int &c0, int &c1) {
    const long long a = (long long)v - reach - lo, b = (long long)v + reach - lo;
    c0 = a <= 0 ? 0 : (int)min((long long)(n - 1), a / (long long)h);
    c1 = b < 0 ? -1 : (int)min((long long)(n - 1), b / (long long)h);
}

// The lane's two points against the wave's list; ex[j]: point j is still exposed.
__device__ __forceinline__ void test_points(const int4 *list, int count, const int off[2][3], bool ex[2]) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the list as every lane wrote it
#pragma unroll 1
    for (int e0 = 0; e0 < count; e0 += 8) {
        if (__builtin_amdgcn_ballot_w64(ex[0] || ex[1]) == 0) break;
        const int e1 = min(e0 + 8, count);
        for (int e = e0; e < e1; e++) {
            const int4 b = list[e];  // one address for the wave: a broadcast
            ex[0] = ex[0] && !sasa_buried(off[0][0], off[0][1], off[0][2], b.x, b.y, b.z, b.w);
            ex[1] = ex[1] && !sasa_buried(off[1][0], off[1][1], off[1][2], b.x, b.y, b.z, b.w);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the list is read before it is written again
}

// Atom `me` (sorted position `self`, or -1 for an atom of the other molecule) against the atoms of grid g, whose cells
// start at s_off[first]: the neighbours are gathered into `list` and the lane's points tested against them.
__device__ __forceinline__ void bury(const Grid &g, const uint32_t *s_off, int first, const int4 *S, const int4 &me, int self,
                                     int e_max, int4 *list, const int off[2][3], bool ex[2], int lane) {
    const int reach = me.w + e_max + kSasaSlack;  // <= the edge of a cell
    int c0[3], c1[3];
    cell_range(me.x, reach, g.lo[0], g.h, g.n[0], c0[0], c1[0]);
    cell_range(me.y, reach, g.lo[1], g.h, g.n[1], c0[1], c1[1]);
    cell_range(me.z, reach, g.lo[2], g.h, g.n[2], c0[2], c1[2]);
    if (c1[2] < c0[2]) return;
    int count = 0;  // uniform
#pragma unroll 1
    for (int cx = c0[0]; cx <= c1[0]; cx++)
#pragma unroll 1
        for (int cy = c0[1]; cy <= c1[1]; cy++) {
            const int row = first + (cx * g.n[1] + cy) * g.n[2];  // consecutive z: consecutive cells, one run of atoms
            const int b0 = (int)s_off[row + c0[2]], b1 = (int)s_off[row + c1[2] + 1];
#pragma unroll 1
            for (int b = b0; b < b1; b += 64) {
                const int i = b + lane;
                bool near = false;
                int4 rel = make_int4(0, 0, 0, 0);
                if (i < b1) {
                    const int4 o = S[i];
                    rel = make_int4(o.x - me.x, o.y - me.y, o.z - me.z, o.w * o.w);
                    const uint32_t lim = (uint32_t)(me.w + o.w + kSasaSlack);
                    near = i != self && square_sum(clamped_abs(rel.x), clamped_abs(rel.y), clamped_abs(rel.z)) < lim * lim;
                }
                const unsigned long long mask = __builtin_amdgcn_ballot_w64(near);
                const int more = __popcll(mask);
                if (count + more > kSasaListCap) {
                    test_points(list, count, off, ex);
                    count = 0;
                }
                if (near)
                    list[count + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u))] = rel;
                count += more;
            }
        }
    test_points(list, count, off, ex);
}

__global__ void __launch_bounds__(kSasaThreads) complex_sasa(ComplexDevice m, SasaDevice d, const double *poses, size_t stride,
                                                            size_t n, char *ws, size_t slot_bytes, unsigned long long *sums,
                                                            uint8_t *free_counts, uint8_t *bound_counts, int *overflow) {
    __shared__ uint32_t s_off[2 * kSasaCells + 1];
    __shared__ int4 s_list[kWaves][kSasaListCap];
    __shared__ int s_box[2][6];  // min x, y, z, max x, y, z of the receptor's and of the ligand's atoms that take part
    __shared__ uint32_t s_wave[kWaves];
    __shared__ unsigned long long s_sums[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int4 *P = reinterpret_cast<int4 *>(ws + (size_t)blockIdx.x * slot_bytes);  // as posed
    int4 *S = P + d.n_part;                                                   // ordered by cell
    int *I = reinterpret_cast<int *>(S + d.n_part);                           // S[i] is atom I[i] of those that take part
    int dir[2][3];
    for (int j = 0; j < 2; j++)
        for (int k = 0; k < 3; k++) dir[j][k] = d_directions[lane + 64 * j][k];
    const uint32_t h0 = (uint32_t)(2 * (d.e_max + kSasaSlack));

    for (size_t pose = blockIdx.x; pose < n; pose += gridDim.x) {
        const double *row = poses + pose * stride;
        for (int i = tid; i < 2 * kSasaCells + 1; i += kSasaThreads) s_off[i] = 0;
        if (tid < 12) s_box[tid / 6][tid % 6] = tid % 6 < 3 ? INT_MAX : INT_MIN;
        if (tid < 4) s_sums[tid] = 0;
        __syncthreads();
#pragma unroll 1
        for (int a = tid; a < d.n_part; a += kSasaThreads) {
            int v[3];
            if (!posed_thousandths(m, row, d.part_atom[a], kComplexCoordBound, v)) *overflow = 1;
            int *box = s_box[a >= d.n_part_rec];
            for (int k = 0; k < 3; k++) {
                atomicMin(&box[k], v[k]);
                atomicMax(&box[3 + k], v[k]);
            }
            P[a] = make_int4(v[0], v[1], v[2], (int)d.part_radius[a] + d.probe);
        }
        __syncthreads();
        const Grid grid[2] = {make_grid(s_box[0], h0), make_grid(s_box[1], h0)};
#pragma unroll 1
        for (int a = tid; a < d.n_part; a += kSasaThreads) {
            const int mol = a >= d.n_part_rec;
            atomicAdd(&s_off[1 + mol * kSasaCells + cell_of(grid[mol], P[a])], 1u);
        }
        __syncthreads();
        {  // exclusive scan of s_off[1 ..]: a run a thread, a wave by shuffles, the waves through LDS
            uint32_t *run = s_off + 1 + tid * kScanRun;
            uint32_t total = 0;
            for (int i = 0; i < kScanRun; i++) total += run[i];
            uint32_t incl = total;
            for (int step = 1; step < 64; step <<= 1) {
                const uint32_t up = __shfl_up(incl, step);
                if (lane >= step) incl += up;
            }
            if (lane == 63) s_wave[wave] = incl;
            __syncthreads();
            uint32_t before = incl - total;
            for (int w = 0; w < wave; w++) before += s_wave[w];
            for (int i = 0; i < kScanRun; i++) {
                const uint32_t c = run[i];
                run[i] = before;
                before += c;
            }
        }
        __syncthreads();
        // the scatter moves every cell's offset to its end: afterwards cell c is s_off[c] .. s_off[c + 1] (s_off[0] = 0)
#pragma unroll 1
        for (int a = tid; a < d.n_part; a += kSasaThreads) {
            const int mol = a >= d.n_part_rec;
            const int4 v = P[a];
            const uint32_t at = atomicAdd(&s_off[1 + mol * kSasaCells + cell_of(grid[mol], v)], 1u);
            S[at] = v;
            I[at] = a;
        }
        __syncthreads();

        // all control flow below is uniform over the wave
        unsigned long long acc[4] = {0, 0, 0, 0};
#pragma unroll 1
        for (int s = wave; s < d.n_part; s += kWaves) {
            const int4 me = S[s];
            const int a = I[s], mol = a >= d.n_part_rec, other = 1 - mol;
            int off[2][3];
            for (int j = 0; j < 2; j++)
                for (int k = 0; k < 3; k++) off[j][k] = sasa_offset(me.w, dir[j][k]);
            bool ex[2] = {true, true};
            bury(grid[mol], s_off, mol * kSasaCells, S, me, s, d.e_max, s_list[wave], off, ex, lane);
            const int n_free = __popcll(__builtin_amdgcn_ballot_w64(ex[0])) + __popcll(__builtin_amdgcn_ballot_w64(ex[1]));
            int n_bound = n_free;
            if (n_free) {
                const int *ob = s_box[other];
                const long long reach = me.w + d.e_max + kSasaSlack;
                const int c[3] = {me.x, me.y, me.z};
                bool meets = true;
                for (int k = 0; k < 3; k++) meets = meets && (long long)ob[k] - c[k] <= reach && (long long)c[k] - ob[3 + k] <= reach;
                if (meets) {
                    bury(grid[other], s_off, other * kSasaCells, S, me, -1, d.e_max, s_list[wave], off, ex, lane);
                    n_bound = __popcll(__builtin_amdgcn_ballot_w64(ex[0])) + __popcll(__builtin_amdgcn_ballot_w64(ex[1]));
                }
            }
            const unsigned long long E2 = (unsigned long long)me.w * (unsigned long long)me.w;
            if (mol == 0) acc[0] += E2 * n_free, acc[1] += E2 * n_bound;
            else acc[2] += E2 * n_free, acc[3] += E2 * n_bound;
            if (free_counts && lane == 0) {
                const size_t at = pose * (size_t)d.n_atoms + d.part_atom[a];
                free_counts[at] = (uint8_t)n_free;
                bound_counts[at] = (uint8_t)n_bound;
            }
        }
        if (lane == 0)
            for (int k = 0; k < 4; k++)
                if (acc[k]) atomicAdd(&s_sums[k], acc[k]);
        __syncthreads();
        if (tid < 4) sums[pose * 4 + tid] = s_sums[tid];
        __syncthreads();  // the slot, the offsets and the sums are reused by the next pose
    }
}

}  // namespace

hipError_t launch_complex_sasa(const ComplexDevice &m, const SasaDevice &d, const double *poses, size_t stride, size_t n,
                               size_t slots, void *ws, unsigned long long *sums, uint8_t *free_counts, uint8_t *bound_counts,
                               int *overflow, hipStream_t stream) {
    hipLaunchKernelGGL(complex_sasa, dim3((unsigned)slots), dim3(kSasaThreads), 0, stream, m, d, poses, stride, n,
                       static_cast<char *>(ws), sasa_slot_bytes(d.n_part), sums, free_counts, bound_counts, overflow);
    return hipGetLastError();
}

}  // namespace ld
