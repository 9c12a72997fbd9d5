// ccs.hip -- K3j: the collision cross-section of every pose by the projection approximation (gfx950; DESIGN §5 K3j;
// lightdock_hip.h, "Collision cross-section").  The kernels and their launchers (kernels/ccs.hpp); the host side is ccs.cpp.
// Discs on a lattice, on the thousandths "%8.3f" prints, all integers.
//   complex_ccs: one workgroup a pose at a time (a launch has at most kCcsSlots workgroups, each with a workspace slot it
//   reuses for pose blockIdx, blockIdx + gridDim, ...):
//     1. every selected atom is posed once (complex_rule.hpp), rounded and kept as int4 (x, y, z, E) in the slot;
//     2. for each of the 64 views the atoms are projected to (a, b, E, first row) into the slot's second half and the
//        extremes of a -+ E, b -+ E are folded by wave into LDS: the view's box of lattice columns and rows;
//     3. the box is cut into pieces of at most kCcsBitmapWords words of LDS, whole rows of 32-column words where a row
//        fits and parts of one row where it does not.  A piece is cleared, then rasterised with work item = (atom, row of
//        the atom): the row's exact half-width w = isqrt(E^2 - dy^2), the columns ceil((a - w) / h) .. floor((a + w) / h)
//        clipped to the piece, ORed word by word with LDS atomics.  Every piece walks every item; an item outside it
//        leaves after two compares.  The count is a popcount over the piece, a wave a row and a lane a word;
//     4. the rigid-receptor form (d.rec_bits): only the ligand is posed and rasterised; the box is the union of the
//        ligand's and the receptor's, and step 3's popcount ORs in the receptor's word, read from the bitmap ccs_receptor
//        made of it once a call.  Words are columns i >> 5 of the lattice itself, so the two bitmaps line up.
// A lattice point is covered or not whatever piece or bitmap holds it, an OR has no order and the counts are integers, so
// a pose's results are the same bits whatever the batch, its place in it, the slot count, the form or the cut.
#include "kernels/ccs.hpp"

#include <climits>

#include "kernels/complex_pose.hpp"

namespace ld {

namespace {

constexpr int kWaves = kCcsThreads / 64;
static_assert(kCcsBitmapWords * sizeof(uint32_t) + 256 <= 64 * 1024, "two workgroups' LDS fit a CU with room to spare");
static_assert((long long)kCcsMaxE * kCcsMaxE < (1 << 24), "ccs_isqrt's float root is exact to one");

__device__ const int32_t d_frames[kCcsViews][6] = {
#include "kernels/ccs_frames.inc"
};

// item -> (item / rmax, item % rmax) for rmax <= 128 and item <= INT_MAX: M = floor((2^32 - 1) / rmax) gives a quotient
// at most one short, the loop puts it right.
__device__ __forceinline__ void split_item(uint32_t item, uint32_t rmax, uint32_t M, int &atom, int &r) {
    uint32_t q = __umulhi(item, M), rest = item - q * rmax;
    while (rest >= rmax) q++, rest -= rmax;
    atom = (int)q;
    r = (int)rest;
}

__device__ __forceinline__ int wave_min(int v) {
    for (int step = 32; step; step >>= 1) v = min(v, __shfl_xor(v, step));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
    for (int step = 32; step; step >>= 1) v = max(v, __shfl_xor(v, step));
    return v;
}

// The rigid receptor, once a call: a workgroup a view, work item = (atom, row of the atom), the spans ORed into global memory.
__global__ void __launch_bounds__(kCcsThreads) ccs_receptor(const int4 *atoms, int n_atoms, int h, int rmax, const CcsRecView *views,
                                                            uint32_t *rec_bits) {
    const int v = blockIdx.x;
    const CcsRecView view = views[v];
    uint32_t *bits = rec_bits + view.offset;
    const uint32_t M = 0xffffffffu / (uint32_t)rmax, items = (uint32_t)n_atoms * (uint32_t)rmax;
#pragma unroll 1
    for (uint32_t item = threadIdx.x; item < items; item += kCcsThreads) {
        int atom, r;
        split_item(item, (uint32_t)rmax, M, atom, r);
        const int4 p = atoms[atom];
        const int a = ccs_project(d_frames[v], p.x, p.y, p.z), b = ccs_project(d_frames[v] + 3, p.x, p.y, p.z);
        const int j = ccs_ceil_div(b - p.w, h) + r;
        int lo, hi;
        if (!ccs_row_span(a, b, p.w, j, h, lo, hi)) continue;
        uint32_t *row = bits + (size_t)(j - view.j0) * (size_t)view.pitch;
        const int w_lo = lo >> 5, w_hi = hi >> 5;
        for (int wc = w_lo; wc <= w_hi; wc++)
            atomicOr(&row[wc - view.wc0], ccs_mask(wc == w_lo ? lo & 31 : 0, wc == w_hi ? hi & 31 : 31));
    }
}

__global__ void __launch_bounds__(kCcsThreads) complex_ccs(ComplexDevice m, CcsDevice d, const double *poses, size_t stride, size_t n,
                                                           char *ws, size_t slot_bytes, uint32_t *counts, unsigned long long *sums,
                                                           int *overflow) {
    __shared__ uint32_t s_bits[kCcsBitmapWords];
    __shared__ int s_box[4];  // min a - E, max a + E, min b - E, max b + E of the view at hand
    __shared__ uint32_t s_wave[kWaves];
    __shared__ int s_bad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int4 *P = reinterpret_cast<int4 *>(ws + (size_t)blockIdx.x * slot_bytes);  // as posed
    int4 *Q = P + d.count;                                                    // as projected: a, b, E, first row
    const bool rigid = d.rec_bits != nullptr;
    const int h = d.h;
    const uint32_t rmax = (uint32_t)d.rmax, M = 0xffffffffu / rmax, items = (uint32_t)d.count * rmax;

    for (size_t pose = blockIdx.x; pose < n; pose += gridDim.x) {
        const double *row = poses + pose * stride;
        if (tid == 0) s_bad = 0;
        __syncthreads();
#pragma unroll 1
        for (int a = tid; a < d.count; a += kCcsThreads) {
            int v[3];
            if (!posed_thousandths(m, row, d.part_atom[d.first + a], kComplexCoordBound, v)) {
                atomicOr(overflow, 1);
                s_bad = 1;
            }
            P[a] = make_int4(v[0], v[1], v[2], (int)d.part_radius[d.first + a] + d.probe);
        }
        __syncthreads();
        bool bad = s_bad != 0;  // uniform, as all control flow below
        unsigned long long total = 0;  // thread 0's
#pragma unroll 1
        for (int v = 0; v < kCcsViews && !bad; v++) {
            if (tid < 4) s_box[tid] = tid & 1 ? INT_MIN : INT_MAX;
            __syncthreads();
            int lo_a = INT_MAX, hi_a = INT_MIN, lo_b = INT_MAX, hi_b = INT_MIN;
#pragma unroll 1
            for (int a = tid; a < d.count; a += kCcsThreads) {
                const int4 p = P[a];
                const int pa = ccs_project(d_frames[v], p.x, p.y, p.z), pb = ccs_project(d_frames[v] + 3, p.x, p.y, p.z);
                Q[a] = make_int4(pa, pb, p.w, ccs_ceil_div(pb - p.w, h));
                lo_a = min(lo_a, pa - p.w), hi_a = max(hi_a, pa + p.w);
                lo_b = min(lo_b, pb - p.w), hi_b = max(hi_b, pb + p.w);
            }
            lo_a = wave_min(lo_a), hi_a = wave_max(hi_a), lo_b = wave_min(lo_b), hi_b = wave_max(hi_b);
            if (lane == 0) {
                atomicMin(&s_box[0], lo_a), atomicMax(&s_box[1], hi_a);
                atomicMin(&s_box[2], lo_b), atomicMax(&s_box[3], hi_b);
            }
            __syncthreads();
            CcsRecView rec = {};
            lo_a = s_box[0], hi_a = s_box[1], lo_b = s_box[2], hi_b = s_box[3];
            if (rigid) {
                rec = d.rec_views[v];
                lo_a = min(lo_a, rec.lo_a), hi_a = max(hi_a, rec.hi_a), lo_b = min(lo_b, rec.lo_b), hi_b = max(hi_b, rec.hi_b);
            }
            const CcsBox box = ccs_box(lo_a, hi_a, lo_b, hi_b, h);
            if (box.columns() * box.rows() > kCcsMaxBox) {
                if (tid == 0) atomicOr(overflow, 2);
                bad = true;
                break;
            }
            const int wc0 = box.wc0(), wc1 = box.wc1();
            const int tw = min(wc1 - wc0 + 1, kCcsBitmapWords), th = kCcsBitmapWords / tw;  // a piece: th rows of tw words
            const uint32_t *rec_bits = rigid ? d.rec_bits + rec.offset : nullptr;
            uint32_t mine = 0;
#pragma unroll 1
            for (int tj = box.j0; tj <= box.j1; tj += th) {
                const int rows = min(th, box.j1 - tj + 1);
#pragma unroll 1
                for (int tc = wc0; tc <= wc1; tc += tw) {
                    const int cols = min(tw, wc1 - tc + 1);
                    for (int k = tid; k < rows * tw; k += kCcsThreads) s_bits[k] = 0;
                    __syncthreads();
#pragma unroll 1
                    for (uint32_t item = tid; item < items; item += kCcsThreads) {
                        int atom, r;
                        split_item(item, rmax, M, atom, r);
                        const int4 q = Q[atom];
                        const int j = q.w + r;
                        if (j < tj || j >= tj + rows) continue;
                        int lo, hi;
                        if (!ccs_row_span(q.x, q.y, q.z, j, h, lo, hi)) continue;
                        const int w_lo = lo >> 5, w_hi = hi >> 5;
                        uint32_t *bits = s_bits + (j - tj) * tw;
                        for (int wc = max(w_lo, tc); wc <= min(w_hi, tc + cols - 1); wc++)
                            atomicOr(&bits[wc - tc], ccs_mask(wc == w_lo ? lo & 31 : 0, wc == w_hi ? hi & 31 : 31));
                    }
                    __syncthreads();
#pragma unroll 1
                    for (int r = wave; r < rows; r += kWaves) {
                        const int j = tj + r;
                        const bool in_rec = rigid && j >= rec.j0 && j < rec.j0 + rec.rows;
                        const uint32_t *rec_row = in_rec ? rec_bits + (size_t)(j - rec.j0) * (size_t)rec.pitch : nullptr;
                        for (int c = lane; c < cols; c += 64) {
                            uint32_t word = s_bits[r * tw + c];
                            const int k = tc + c - rec.wc0;
                            if (in_rec && k >= 0 && k < rec.pitch) word |= rec_row[k];
                            mine += (uint32_t)__popc(word);
                        }
                    }
                    __syncthreads();  // the piece is counted before the next one clears it
                }
            }
            for (int step = 32; step; step >>= 1) mine += __shfl_xor(mine, step);
            if (lane == 0) s_wave[wave] = mine;
            __syncthreads();
            if (tid == 0) {
                uint32_t count = 0;
                for (int w = 0; w < kWaves; w++) count += s_wave[w];
                counts[pose * kCcsViews + v] = count;
                total += count;
            }
            __syncthreads();  // the box, the wave counts and the slot's projections are reused by the next view
        }
        if (tid == 0 && !bad) sums[pose] = total;
        __syncthreads();  // the slot is reused by the next pose
    }
}

}  // namespace

hipError_t launch_ccs_receptor(const int4 *atoms, int n_atoms, int h, int rmax, const CcsRecView *views, uint32_t *rec_bits,
                               hipStream_t stream) {
    hipLaunchKernelGGL(ccs_receptor, dim3(kCcsViews), dim3(kCcsThreads), 0, stream, atoms, n_atoms, h, rmax, views, rec_bits);
    return hipGetLastError();
}

hipError_t launch_complex_ccs(const ComplexDevice &m, const CcsDevice &d, const double *poses, size_t stride, size_t n, size_t slots,
                              void *ws, uint32_t *counts, unsigned long long *sums, int *overflow, hipStream_t stream) {
    hipLaunchKernelGGL(complex_ccs, dim3((unsigned)slots), dim3(kCcsThreads), 0, stream, m, d, poses, stride, n, static_cast<char *>(ws),
                       ccs_slot_bytes(d.count), counts, sums, overflow);
    return hipGetLastError();
}

}  // namespace ld
