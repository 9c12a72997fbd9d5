// emfit.hip -- K3i: the density every pose would show in a map, and its exact sums against the map (gfx950; DESIGN §5
// K3i; lightdock_hip.h, "Density fit").  The kernels and their launchers (kernels/emfit.hpp); the host side is emfit.cpp.
// Everything is integers on the thousandths "%8.3f" prints; the device evaluates no exp.
//   emfit_init: every pose's row of sums starts from the base row (the rigid receptor's) or 0, its box empty.
//   emfit_fill: every pose's output grid starts from the base grid or 0 (ld_complex_simulate_density only).
//   emfit_pose: a thread an atom that takes part and a pose: posed (complex_rule.hpp), rounded, kept as int4 (x, y, z,
//     weight).  The workgroup's box and its count of atoms in no voxel's cell meet in LDS and go out as one atomic each.
//   emfit_list: a workgroup a pose turns the pose's box, widened by the table's reach, into a box of bricks and appends
//     (pose, brick) items to one list.  The list, not the grid, sizes the work that follows.
//   emfit_bricks: a fixed number of workgroups share the list.  For an item the workgroup holds the brick's 16 x 16 x 4 voxels in
//     registers, a thread a column of 4 along z, started from the base grid or 0.  It walks the pose's atoms a tile of 256
//     at a time: a thread tests one atom's support box against the brick and the hits are compacted in LDS; every thread then
//     reads the hits (broadcast reads) and gathers: x^2 + y^2 once an atom, then 4 voxels of 32-bit work each, the table a
//     byte read from LDS.  No atomics touch a voxel.  The brick's four sums are reduced by shuffles and LDS and meet the
//     pose's row as global integer atomics, less the base's sums of that brick when the row started from the base's totals.
// Integer adds are order-free, so a pose's words are the same whatever the batch, its place in it or the chunk.
#include "kernels/emfit.hpp"

#include <climits>

#include "kernels/complex_pose.hpp"

namespace ld {

namespace {

static_assert(kEmfitThreads == 256, "four waves; the reduction below counts on it");
static_assert(2ll * kComplexCoordBound + 2ll * kEmfitMaxAxis * kEmfitMaxStep < (1ll << 31), "a coordinate less a voxel's centre fits an int32");

__global__ void __launch_bounds__(256) emfit_init(ld_density_sums *rows, EmfitBox *boxes, const ld_density_sums *from, size_t n) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    ld_density_sums r = {0, 0, 0, 0, 0, 0};
    if (from) r = *from;
    rows[p] = r;
    EmfitBox b;
    for (int k = 0; k < 3; k++) b.lo[k] = INT_MAX, b.hi[k] = INT_MIN;
    boxes[p] = b;
}

__global__ void __launch_bounds__(256) emfit_fill(uint32_t *grid, const uint32_t *base, size_t n, size_t voxels) {
    const size_t total = n * voxels;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) grid[i] = base ? base[i % voxels] : 0u;
}

__global__ void __launch_bounds__(kEmfitPoseThreads) emfit_pose(ComplexDevice m, SaxsDevice d, EmfitMap map, const double *poses, size_t stride,
                                                                int first, int count, int4 *out, size_t out_stride, EmfitBox *boxes,
                                                                ld_density_sums *rows, int *overflow) {
    __shared__ int s_lo[3], s_hi[3], s_outside;
    const int a = blockIdx.x * kEmfitPoseThreads + threadIdx.x;
    const size_t pose = blockIdx.y;
    if (threadIdx.x < 3) s_lo[threadIdx.x] = INT_MAX, s_hi[threadIdx.x] = INT_MIN;
    if (threadIdx.x == 3) s_outside = 0;
    __syncthreads();
    if (a < count) {
        int v[3];
        if (!posed_thousandths(m, poses + pose * stride, d.part_atom[first + a], kComplexCoordBound, v)) *overflow = 1;
        bool outside = false;
        for (int k = 0; k < 3; k++) {
            atomicMin(&s_lo[k], v[k]);
            atomicMax(&s_hi[k], v[k]);
            outside |= emfit_axis_outside(v[k], map.origin[k], map.step[k], map.n[k]);
        }
        if (outside) atomicAdd(&s_outside, 1);
        out[pose * out_stride + a] = make_int4(v[0], v[1], v[2], (int)emfit_weight(d.part_class[first + a]));
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        atomicMin(&boxes[pose].lo[threadIdx.x], s_lo[threadIdx.x]);
        atomicMax(&boxes[pose].hi[threadIdx.x], s_hi[threadIdx.x]);
    }
    if (threadIdx.x == 3 && s_outside) atomicAdd(&rows[pose].outside, (uint32_t)s_outside);
}

__global__ void __launch_bounds__(kEmfitListThreads) emfit_list(EmfitMap map, uint32_t reach, const EmfitBox *boxes, uint2 *items, uint32_t *n_items) {
    __shared__ uint32_t s_at;
    const size_t pose = blockIdx.x;
    const EmfitBox box = boxes[pose];
    int lo[3], hi[3];
    for (int k = 0; k < 3; k++) {
        if (box.lo[k] > box.hi[k]) return;  // no atom was posed: uniform
        emfit_axis_range(box.lo[k], box.hi[k], reach, map.origin[k], map.step[k], map.n[k], &lo[k], &hi[k]);
        if (lo[k] > hi[k]) return;  // the supports miss the grid: uniform
        lo[k] /= EmfitMap::brick_size(k), hi[k] /= EmfitMap::brick_size(k);
    }
    const int ex = hi[0] - lo[0] + 1, ey = hi[1] - lo[1] + 1, ez = hi[2] - lo[2] + 1;
    const uint32_t total = (uint32_t)ex * ey * ez;
    if (threadIdx.x == 0) s_at = atomicAdd(n_items, total);
    __syncthreads();
    const uint32_t at = s_at;
    for (uint32_t i = threadIdx.x; i < total; i += kEmfitListThreads) {
        const int bx = lo[0] + (int)(i % ex), by = lo[1] + (int)(i / ex % ey), bz = lo[2] + (int)(i / ex / ey);
        items[at + i] = make_uint2((uint32_t)pose, (uint32_t)((bz * map.bricks(1) + by) * map.bricks(0) + bx));
    }
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(kEmfitThreads) emfit_bricks(EmfitBricks b) {
    __shared__ int4 s_hit[kEmfitThreads];
    __shared__ uint8_t s_K[kEmfitMaxTable];
    __shared__ int s_count;
    __shared__ unsigned long long s_part[kEmfitThreads / 64][4];
    const int tid = threadIdx.x, ci = tid % kEmfitBrick, cj = tid / kEmfitBrick;
    for (uint32_t t = tid; t < b.table.length; t += kEmfitThreads) s_K[t] = b.table.K[t];
    const uint32_t n_items = *b.n_items, shift = b.table.shift, limit = b.table.limit, reach = b.table.reach;
    const int nbx = b.map.bricks(0), nby = b.map.bricks(1);
    const size_t voxels = b.map.voxels(), plane = (size_t)b.map.n[0] * b.map.n[1];
    bool over = false;
#pragma unroll 1
    for (uint32_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const uint2 it = b.items[item];
        const size_t pose = it.x;
        const int brick = (int)it.y;
        const int i0 = brick % nbx * kEmfitBrick, j0 = brick / nbx % nby * kEmfitBrick, k0 = brick / nbx / nby * kEmfitDepth;
        // the part of the brick inside the grid: 1 .. 16 voxels on x and y, 1 .. kEmfitDepth on z
        const int ex = min(kEmfitBrick, b.map.n[0] - i0), ey = min(kEmfitBrick, b.map.n[1] - j0), ez = min(kEmfitDepth, b.map.n[2] - k0);
        const int X0 = b.map.origin[0] + i0 * b.map.step[0], Y0 = b.map.origin[1] + j0 * b.map.step[1], Z0 = b.map.origin[2] + k0 * b.map.step[2];
        const int X1 = X0 + (ex - 1) * b.map.step[0], Y1 = Y0 + (ey - 1) * b.map.step[1], Z1 = Z0 + (ez - 1) * b.map.step[2];
        const bool column = ci < ex && cj < ey;  // this thread's column lies in the grid
        const size_t v0 = (size_t)k0 * plane + (size_t)(j0 + cj) * b.map.n[0] + (size_t)(i0 + ci);
        const int x = X0 + ci * b.map.step[0], y = Y0 + cj * b.map.step[1], hz = b.map.step[2];
        uint32_t acc[kEmfitDepth];
#pragma unroll
        for (int k = 0; k < kEmfitDepth; k++) acc[k] = (b.base && column && k < ez) ? b.base[v0 + (size_t)k * plane] : 0u;
        const int4 *atoms = b.atoms + pose * b.atom_stride;
#pragma unroll 1
        for (int a0 = 0; a0 < b.n_atoms; a0 += kEmfitThreads) {
            if (tid == 0) s_count = 0;
            __syncthreads();  // the zeroed count, the table; the last tile's readers are past their hits
            if (a0 + tid < b.n_atoms) {
                const int4 v = atoms[a0 + tid];
                // an atom beyond reach of the brick on an axis adds to none of its voxels (|coordinate| <= 10^9, reach < 2^16)
                if (v.x + (int)reach >= X0 && v.x - (int)reach <= X1 && v.y + (int)reach >= Y0 && v.y - (int)reach <= Y1 &&
                    v.z + (int)reach >= Z0 && v.z - (int)reach <= Z1)
                    s_hit[atomicAdd(&s_count, 1)] = v;
            }
            __syncthreads();
            const int hits = s_count;
#pragma unroll 1
            for (int h = 0; h < hits; h++) {
                const int4 v = s_hit[h];
                const uint32_t ax = emfit_abs(x - v.x), ay = emfit_abs(y - v.y);
                if (ax > reach || ay > reach) continue;
                const unsigned long long xy = (unsigned long long)ax * ax + (unsigned long long)ay * ay;
                if (xy >= limit) continue;
                const uint32_t low = (uint32_t)xy, room = limit - low;  // z^2 < room <=> d2 < limit, all below 2^32
                const uint32_t w = (uint32_t)v.w;
                const int dz = Z0 - v.z;
#pragma unroll
                for (int k = 0; k < kEmfitDepth; k++) {
                    const uint32_t az = emfit_abs(dz + k * hz);
                    const uint32_t zz = az * az;  // used only when az <= reach < 2^16
                    if (az <= reach && zz < room) acc[k] += w * s_K[(low + zz) >> shift];
                }
            }
            __syncthreads();
        }
        unsigned long long s = 0, ss = 0, se = 0, in = 0;
        if (column) {
#pragma unroll
            for (int k = 0; k < kEmfitDepth; k++) {
                if (k < ez) {
                    const uint32_t v = acc[k], e = b.map.E[v0 + (size_t)k * plane];
                    over |= v >= kEmfitVoxelLimit;
                    s += v;
                    ss += (unsigned long long)v * v;
                    se += (unsigned long long)v * e;
                    in += e ? v : 0u;
                    if (b.grid) b.grid[pose * voxels + v0 + (size_t)k * plane] = v;
                }
            }
        }
        s = wave_sum(s), ss = wave_sum(ss), se = wave_sum(se), in = wave_sum(in);
        if (tid % 64 == 0) {
            unsigned long long *part = s_part[tid / 64];
            part[0] = s, part[1] = ss, part[2] = se, part[3] = in;
        }
        __syncthreads();
        if (tid < 4) {
            unsigned long long sum = s_part[0][tid] + s_part[1][tid] + s_part[2][tid] + s_part[3][tid];
            if (b.brick_sums) b.brick_sums[(size_t)brick * 4 + tid] = sum;
            if (b.base_sums) sum -= b.base_sums[(size_t)brick * 4 + tid];  // modulo 2^64: the row holds the base's total
            ld_density_sums *row = b.rows + pose;
            unsigned long long *word = reinterpret_cast<unsigned long long *>(tid == 0 ? &row->s : tid == 1 ? &row->ss : tid == 2 ? &row->se : &row->inside_sum);
            if (sum) __hip_atomic_fetch_add(word, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();  // s_part is read before the next item writes it
    }
    if (over) *b.overflow = 1;
}

}  // namespace

hipError_t launch_emfit_init(ld_density_sums *rows, EmfitBox *boxes, const ld_density_sums *from, size_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(emfit_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, rows, boxes, from, n);
    return hipGetLastError();
}

hipError_t launch_emfit_fill(uint32_t *grid, const uint32_t *base, size_t n, size_t voxels, hipStream_t stream) {
    if (n == 0 || voxels == 0) return hipSuccess;
    const size_t blocks = (n * voxels + 255) / 256;
    hipLaunchKernelGGL(emfit_fill, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, stream, grid, base, n, voxels);
    return hipGetLastError();
}

hipError_t launch_emfit_pose(const ComplexDevice &m, const SaxsDevice &d, const EmfitMap &map, const double *poses, size_t stride, size_t n,
                             int first, int count, int4 *out, size_t out_stride, EmfitBox *boxes, ld_density_sums *rows, int *overflow,
                             hipStream_t stream) {
    if (n == 0 || count <= 0) return hipSuccess;
    if (n > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(emfit_pose, dim3((unsigned)((count + kEmfitPoseThreads - 1) / kEmfitPoseThreads), (unsigned)n), dim3(kEmfitPoseThreads), 0,
                       stream, m, d, map, poses, stride, first, count, out, out_stride, boxes, rows, overflow);
    return hipGetLastError();
}

hipError_t launch_emfit_list(const EmfitMap &map, uint32_t reach, const EmfitBox *boxes, size_t n, uint2 *items, uint32_t *n_items,
                             hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(emfit_list, dim3((unsigned)n), dim3(kEmfitListThreads), 0, stream, map, reach, boxes, items, n_items);
    return hipGetLastError();
}

hipError_t launch_emfit_bricks(const EmfitBricks &b, size_t groups, hipStream_t stream) {
    if (groups == 0) return hipSuccess;
    if (b.table.length < 1 || b.table.length > (uint32_t)kEmfitMaxTable || groups > (size_t)kEmfitMaxGroups) return hipErrorInvalidValue;
    hipLaunchKernelGGL(emfit_bricks, dim3((unsigned)groups), dim3(kEmfitThreads), 0, stream, b);
    return hipGetLastError();
}

}  // namespace ld
