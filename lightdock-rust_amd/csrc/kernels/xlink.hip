// xlink.hip -- K3k: the cross-links of every pose (gfx950; lightdock_hip.h, "Cross-links").  The kernels
// and their launchers (kernels/xlink.hpp); the host side is xlink.cpp.  Shortest paths on a lattice, on the thousandths
// "%8.3f" prints, all integers.
//   xlink_straight: a thread a (pose, link): both anchors posed (complex_rule.hpp), |c_a - c_b|^2 in 64 bits.
//   xlink_paths: one workgroup a job (pose, source anchor) at a time (a launch has at most kXlinkSlots workgroups, each
//   with a workspace slot it reuses for job blockIdx, blockIdx + gridDim, ...):
//     1. the source anchor is posed; its box of nodes within M an axis is the search box (xlink_box);
//     2. every blocker is posed and rounded; those whose sphere reaches into the box are kept as int4 (x, y, z, E) in the
//        slot, in any order;
//     3. the blocked bits of the box are cleared and rasterised with work item = (blocker, lattice row of the blocker):
//        the row's exact span of blocked nodes (xlink_row_span) clipped to the box, ORed word by word with atomics -- in
//        LDS when the box's bits fit kXlinkLdsWords, in the slot otherwise;
//     4. the 16-bit field of the box is set to "not reached", then every door of the source takes its hop;
//     5. level k = 0, 1, ... floor(M / h) settles the nodes whose distance lies in [k h, (k + 1) h): every free node not yet
//        below k h takes the minimum of its own word (a door's hop) and, over its 26 neighbours whose word is below k h
//        (settled, final), of that word plus the move's weight, and keeps it if it is below (k + 1) h.  Every weight is >= h,
//        so the best predecessor of such a node was settled before the level began: no word written in a level is read
//        in it, the sweep needs no atomics and its result does not depend on the order of the threads.  A level scans only
//        the nodes an axis of which is less than (k + 1) h from the source (a hop is at least its extent on an axis, a
//        move's weight at least h).  Two levels in a row that settle nothing, past the last door's hop, end the sweep: a
//        predecessor is at most w3 < 2 h below;
//     6. every link of the source: the other anchor is posed and its doors' minimum of word + hop is folded by wave, then
//        through LDS.
// The field is a unique fixed point, so a pose's results are the same bits whatever the batch, its place in it, the slot
// count, the grouping of the links or the schedule.
#include "kernels/xlink.hpp"

#include <climits>

#include "kernels/complex_pose.hpp"

namespace ld {

namespace {

static_assert(kXlinkLdsWords * sizeof(uint32_t) + 256 <= 64 * 1024, "two workgroups' LDS fit a CU with room to spare");
static_assert(kXlinkMaxLength + kXlinkMaxCell + 3465 < kXlinkUnreached, "a settled word plus w3 is below the 'not reached' word");

__global__ void __launch_bounds__(256) xlink_straight(ComplexDevice m, const double *poses, size_t stride, size_t n, const uint32_t *links,
                                                      int n_links, unsigned long long *straight2, int *overflow) {
    const size_t item = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (item >= n * (size_t)n_links) return;
    const size_t pose = item / (size_t)n_links, l = item % (size_t)n_links;
    const double *row = poses + pose * stride;
    int a[3], b[3];
    const bool ok_a = posed_thousandths(m, row, links[2 * l], kComplexCoordBound, a);
    const bool ok_b = posed_thousandths(m, row, links[2 * l + 1], kComplexCoordBound, b);
    if (!ok_a || !ok_b) {
        atomicOr(overflow, 1);
        return;
    }
    straight2[item] = xlink_square(a, b);
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
    for (int step = 32; step; step >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, step));
    return v;
}

// The bits lo .. hi (of the padded box) set in `bits`.
__device__ __forceinline__ void set_bits(uint32_t *bits, int lo, int hi) {
    const int w_lo = lo >> 5, w_hi = hi >> 5;
    for (int w = w_lo; w <= w_hi; w++) atomicOr(&bits[w], ccs_mask(w == w_lo ? lo & 31 : 0, w == w_hi ? hi & 31 : 31));
}

__device__ __forceinline__ bool blocked(const uint32_t *bits, int idx) { return bits[idx >> 5] >> (idx & 31) & 1; }

// One job with its source anchor posed at c (s_c), everything below uniform across the workgroup.  `bits`: LDS or the slot's.
__device__ __forceinline__ void search(const ComplexDevice &m, const XlinkDevice &d, const double *row, size_t pose, int source, int4 *B,
                                       uint16_t *F, uint32_t *bits, uint32_t *path, int *overflow, const int *s_c, int *s_n, int *s_t,
                                       uint32_t *s_best, int *s_bad) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int h = d.h, M = d.M, reach = d.reach;
    const int c[3] = {s_c[0], s_c[1], s_c[2]};
    const XlinkBox box = xlink_box(c, M, h);
    const int px = box.px(), py = box.py(), plane = px * py, padded = box.padded();

    // 2. the blockers that reach into the box
#pragma unroll 1
    for (int a = tid; a < d.n_part; a += kXlinkThreads) {
        int v[3];
        if (!posed_thousandths(m, row, d.part_atom[a], kComplexCoordBound, v)) {
            atomicOr(overflow, 1);
            *s_bad = 1;
        }
        const int E = (int)d.part_radius[a] + d.probe;
        bool in = true;
        for (int k = 0; k < 3; k++) {
            const long long lo = (long long)box.lo[k] * h, hi = (long long)(box.lo[k] + box.n[k] - 1) * h;
            in = in && (long long)v[k] + E > lo && (long long)v[k] - E < hi;
        }
        if (in) B[atomicAdd(s_n, 1)] = make_int4(v[0], v[1], v[2], E);
    }
    // 3. the blocked bits; 4. the field
    const int words = (padded + 31) >> 5;
    for (int w = tid; w < words; w += kXlinkThreads) bits[w] = 0;
    uint32_t *F32 = reinterpret_cast<uint32_t *>(F);
    for (int w = tid; w < (padded + 1) >> 1; w += kXlinkThreads) F32[w] = 0xFFFFFFFFu;
    __syncthreads();
    if (*s_bad) return;
    const int rmax = d.rmax, rows = rmax * rmax, items = *s_n * rows;  // n_part * rmax^2 <= INT_MAX: the host's check
#pragma unroll 1
    for (int item = tid; item < items; item += kXlinkThreads) {
        const int atom = item / rows, r = item - atom * rows, rj = r / rmax, rk = r - rj * rmax;
        const int4 p = B[atom];
        const int j = ccs_ceil_div(p.y - (p.w - 1), h) + rj - box.lo[1], k = ccs_ceil_div(p.z - (p.w - 1), h) + rk - box.lo[2];
        if (j < 0 || j >= box.n[1] || k < 0 || k >= box.n[2]) continue;
        int lo, hi;
        if (!xlink_row_span(p.x, p.y, p.z, p.w, (long long)(j + box.lo[1]) * h, (long long)(k + box.lo[2]) * h, h, lo, hi)) continue;
        lo = max(lo - box.lo[0], 0), hi = min(hi - box.lo[0], box.n[0] - 1);
        if (lo > hi) continue;
        const int base = box.index(0, j, k);
        set_bits(bits, base + lo, base + hi);
    }
    __syncthreads();
    // the doors of the source: the free nodes within the reach, each with its hop
    {
        int lo[3], n[3];
        for (int k = 0; k < 3; k++) {
            lo[k] = max(ccs_ceil_div(c[k] - reach, h), box.lo[k]);
            n[k] = min(ccs_floor_div(c[k] + reach, h), box.lo[k] + box.n[k] - 1) - lo[k] + 1;
        }
        const int total = n[0] > 0 && n[1] > 0 && n[2] > 0 ? n[0] * n[1] * n[2] : 0;
        const long long reach2 = (long long)reach * reach;
#pragma unroll 1
        for (int t = tid; t < total; t += kXlinkThreads) {
            const int i = lo[0] + t % n[0], r = t / n[0], j = lo[1] + r % n[1], k = lo[2] + r / n[1];
            const long long dx = (long long)i * h - c[0], dy = (long long)j * h - c[1], dz = (long long)k * h - c[2];
            const long long d2 = dx * dx + dy * dy + dz * dz;
            if (d2 > reach2) continue;
            const int idx = box.index(i - box.lo[0], j - box.lo[1], k - box.lo[2]);
            if (blocked(bits, idx)) continue;
            F[idx] = (uint16_t)xlink_isqrt(d2);
            *s_t = 1;  // the source has a door
        }
    }
    __syncthreads();
    // 5. the levels
    if (*s_t) {
        int fc[3];
        for (int k = 0; k < 3; k++) fc[k] = ccs_floor_div(c[k], h) - box.lo[k];
        const int w1 = h, w2 = d.w2, w3 = d.w3;
        int idle = 0;
#pragma unroll 1
        for (int level = 0; level <= M / h; level++) {
            const int below = level * h, limit = below + h;
            int lo[3], n[3];
            for (int k = 0; k < 3; k++) {
                lo[k] = max(fc[k] - level, 0);
                n[k] = min(fc[k] + level + 1, box.n[k] - 1) - lo[k] + 1;
            }
            const int total = n[0] * n[1] * n[2];  // every n >= 1: the source's own cell is inside the box
            int settled = 0;
#pragma unroll 1
            for (int t = tid; t < total; t += kXlinkThreads) {
                const int i = lo[0] + t % n[0], r = t / n[0], j = lo[1] + r % n[1], k = lo[2] + r / n[1];
                const int idx = box.index(i, j, k);
                const int own = F[idx];
                if (own < below || blocked(bits, idx)) continue;
                int best = own;
#pragma unroll
                for (int dz = -1; dz <= 1; dz++)
#pragma unroll
                    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                        for (int dx = -1; dx <= 1; dx++) {
                            const int moves = (dx != 0) + (dy != 0) + (dz != 0);
                            if (moves == 0) continue;
                            const int u = F[idx + dz * plane + dy * px + dx];
                            if (u < below) best = min(best, u + (moves == 1 ? w1 : moves == 2 ? w2 : w3));
                        }
                if (best < limit) {
                    if (best != own) F[idx] = (uint16_t)best;
                    settled = 1;
                }
            }
            idle = __syncthreads_or(settled) ? 0 : idle + 1;  // the level's words are written before the next reads them
            if (idle >= 2 && below > reach) break;
        }
    }
    // 6. the links of the source
#pragma unroll 1
    for (uint32_t e = d.first[source]; e < d.first[source + 1]; e++) {
        __syncthreads();  // s_t and s_best are free
        if (tid == 0) {
            int v[3];
            if (!posed_thousandths(m, row, d.target[e], kComplexCoordBound, v)) {
                atomicOr(overflow, 1);
                *s_bad = 1;
            }
            s_t[0] = v[0], s_t[1] = v[1], s_t[2] = v[2];
            *s_best = kXlinkNoPath;
        }
        __syncthreads();
        if (*s_bad) return;
        const int b[3] = {s_t[0], s_t[1], s_t[2]};
        int lo[3], n[3];
        for (int k = 0; k < 3; k++) {
            lo[k] = max(ccs_ceil_div(b[k] - reach, h), box.lo[k]);
            n[k] = min(ccs_floor_div(b[k] + reach, h), box.lo[k] + box.n[k] - 1) - lo[k] + 1;
        }
        const int total = n[0] > 0 && n[1] > 0 && n[2] > 0 ? n[0] * n[1] * n[2] : 0;
        const long long reach2 = (long long)reach * reach;
        uint32_t best = kXlinkNoPath;
#pragma unroll 1
        for (int t = tid; t < total; t += kXlinkThreads) {
            const int i = lo[0] + t % n[0], r = t / n[0], j = lo[1] + r % n[1], k = lo[2] + r / n[1];
            const long long dx = (long long)i * h - b[0], dy = (long long)j * h - b[1], dz = (long long)k * h - b[2];
            const long long d2 = dx * dx + dy * dy + dz * dz;
            if (d2 > reach2) continue;
            const uint32_t word = F[box.index(i - box.lo[0], j - box.lo[1], k - box.lo[2])];  // a blocked node was never reached
            if (word != kXlinkUnreached) best = min(best, word + (uint32_t)xlink_isqrt(d2));
        }
        best = wave_min(best);
        if (lane == 0 && best != kXlinkNoPath) atomicMin(s_best, best);
        __syncthreads();
        if (tid == 0) path[pose * (size_t)d.n_links + d.link[e]] = *s_best <= (uint32_t)M ? *s_best : kXlinkNoPath;
    }
}

__global__ void __launch_bounds__(kXlinkThreads) xlink_paths(ComplexDevice m, XlinkDevice d, const double *poses, size_t stride, size_t n,
                                                             char *ws, size_t slot_bytes, size_t field_offset, size_t bits_offset,
                                                             int bits_in_lds, uint32_t *path, int *overflow) {
    __shared__ uint32_t s_bits[kXlinkLdsWords];
    __shared__ int s_c[3], s_t[3], s_n, s_bad;
    __shared__ uint32_t s_best;
    char *slot = ws + (size_t)blockIdx.x * slot_bytes;
    int4 *B = reinterpret_cast<int4 *>(slot);
    uint16_t *F = reinterpret_cast<uint16_t *>(slot + field_offset);
    uint32_t *g_bits = reinterpret_cast<uint32_t *>(slot + bits_offset);
    const size_t jobs = n * (size_t)d.n_sources;
    for (size_t job = blockIdx.x; job < jobs; job += gridDim.x) {
        const size_t pose = job / (size_t)d.n_sources;
        const int source = (int)(job % (size_t)d.n_sources);
        const double *row = poses + pose * stride;
        __syncthreads();  // the slot and the shared words are free
        if (threadIdx.x == 0) {
            int v[3];
            s_bad = 0, s_n = 0, s_t[0] = 0;
            if (!posed_thousandths(m, row, d.source[source], kComplexCoordBound, v)) {
                atomicOr(overflow, 1);
                s_bad = 1;
            }
            s_c[0] = v[0], s_c[1] = v[1], s_c[2] = v[2];
        }
        __syncthreads();
        if (s_bad) continue;
        if (bits_in_lds)
            search(m, d, row, pose, source, B, F, s_bits, path, overflow, s_c, &s_n, s_t, &s_best, &s_bad);
        else
            search(m, d, row, pose, source, B, F, g_bits, path, overflow, s_c, &s_n, s_t, &s_best, &s_bad);
    }
}

}  // namespace

hipError_t launch_xlink_straight(const ComplexDevice &m, const double *poses, size_t stride, size_t n, const uint32_t *links, int n_links,
                                 unsigned long long *straight2, int *overflow, hipStream_t stream) {
    const size_t items = n * (size_t)n_links;
    hipLaunchKernelGGL(xlink_straight, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, stream, m, poses, stride, n, links, n_links,
                       straight2, overflow);
    return hipGetLastError();
}

hipError_t launch_xlink_paths(const ComplexDevice &m, const XlinkDevice &d, const double *poses, size_t stride, size_t n, size_t slots,
                              void *ws, uint32_t *path, int *overflow, hipStream_t stream) {
    hipLaunchKernelGGL(xlink_paths, dim3((unsigned)slots), dim3(kXlinkThreads), 0, stream, m, d, poses, stride, n, static_cast<char *>(ws),
                       xlink_slot_bytes(d.n_part, d.M, d.h), xlink_field_offset(d.n_part), xlink_bits_offset(d.n_part, d.M, d.h),
                       xlink_bits_in_lds(d.M, d.h) ? 1 : 0, path, overflow);
    return hipGetLastError();
}

}  // namespace ld
