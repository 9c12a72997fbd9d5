// saxs.hip -- K3h: the pair-distance histogram of every pose by pair class, and the Debye sum over it (gfx950; DESIGN §5
// K3h; lightdock_hip.h, "Small-angle scattering").  The kernels and their launchers (kernels/saxs.hpp); the host side is
// saxs.cpp.  The histogram is exact integers on the thousandths "%8.3f" prints; the Debye sum is f64 in a fixed order.
//   saxs_pose: a thread an atom that takes part and a pose: posed (complex_rule.hpp), rounded, kept as int4 (x, y, z, class).
//   saxs_rows: every pose's row of counts starts from the base row (the receptor's own pairs when it has no modes) or 0.
//   saxs_histogram: a workgroup takes one pose and a range of the tile pairs (ta <= tb, tb-major, tiles of kSaxsTile
//     atoms).  Its 21 x bins words are in LDS.  The b-tile is in LDS; a lane of either half of the workgroup holds one
//     a-atom in registers and walks its half of the b-tile, a broadcast read an atom.  The bin is the floor of the f32
//     estimate of d / w (v_sqrt_f32; kernels/saxs.hpp derives its error) unless that lies within kSaxsEdge of a bin's
//     edge: then d^2 in 64 bits and the two compares of saxs_bin decide, about one pair in five hundred.  Adds are LDS
//     integer atomics that return nothing; the non-zero words meet the pose's row with global integer atomics.  A pair
//     counts when a < b and b >= first_b.
//   saxs_debye: a workgroup a pose stages the row in LDS; a thread a q_j keeps the 21 sums G_c over k ascending (one
//     read of s(q_j r_k) a bin, consecutive threads consecutive words) and then adds F_{j,c} G_c to S_j, c ascending.
// Integer adds are order-free, and every f64 sum has one order, so a pose's results are the same bits whatever the batch,
// its place in it, the split or the chunk.
#include "kernels/saxs.hpp"

#include <type_traits>

#include "kernels/complex_pose.hpp"

namespace ld {

namespace {

static_assert(kSaxsThreads == 2 * kSaxsTile, "two halves, an a-atom a lane of each");
static_assert((unsigned long long)kSaxsMaxBins * kSaxsMaxWidth < kSaxsAxisClamp, "a clamped axis is beyond the last bin");
static_assert(2ll * kComplexCoordBound < (1ll << 31), "the difference of two coordinates fits an int32");

__global__ void __launch_bounds__(kSaxsPoseThreads) saxs_pose(ComplexDevice m, SaxsDevice d, const double *poses, size_t stride,
                                                              int first, int count, int4 *out, size_t out_stride, int *overflow) {
    const int a = blockIdx.x * kSaxsPoseThreads + threadIdx.x;
    if (a >= count) return;
    const size_t pose = blockIdx.y;
    int v[3];
    if (!posed_thousandths(m, poses + pose * stride, d.part_atom[first + a], kComplexCoordBound, v)) *overflow = 1;
    out[pose * out_stride + a] = make_int4(v[0], v[1], v[2], (int)d.part_class[first + a]);
}

__global__ void __launch_bounds__(256) saxs_rows(const uint32_t *base, uint32_t *rows, size_t n, size_t row_words) {
    const size_t total = n * row_words;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) rows[i] = base ? base[i % row_words] : 0u;
}

__global__ void __launch_bounds__(kSaxsThreads) saxs_histogram(SaxsHistogram h) {
    extern __shared__ uint32_t s_hist[];  // 21 x bins, and a spare word that takes the adds of pairs beyond the last bin
    __shared__ int4 s_b[kSaxsTile];
    const int tid = threadIdx.x, half = tid / kSaxsTile, lane_atom = tid % kSaxsTile;
    const size_t pose = blockIdx.y;
    const int4 *atoms = h.atoms + pose * h.atom_stride;
    const int words = kSaxsPairClasses * h.bins;
    for (int i = tid; i < words; i += kSaxsThreads) s_hist[i] = 0;

    // the range of tile pairs, tb-major from the tile that holds first_b: all uniform
    const int nt = (h.n_atoms + kSaxsTile - 1) / kSaxsTile, t0 = h.first_b / kSaxsTile;
    const long long total = (long long)nt * (nt + 1) / 2 - (long long)t0 * (t0 + 1) / 2;
    long long p = total * blockIdx.x / h.splits;
    const long long p_end = total * (blockIdx.x + 1) / h.splits;
    int tb = t0, ta = 0;
    {
        long long skip = p;
        while (tb < nt && skip >= tb + 1) skip -= tb + 1, tb++;
        ta = (int)skip;
    }
    const float inv_w = 1.0f / (float)h.width;
    const uint32_t w = h.width, bins = (uint32_t)h.bins;
    int loaded = -1;
    bool over = false;
#pragma unroll 1
    for (; p < p_end; p++) {
        if (loaded != tb) {
            __syncthreads();  // the zeroed words; the last tile's readers
            const int b = tb * kSaxsTile + tid;
            if (tid < kSaxsTile && b < h.n_atoms) {
                int4 v = atoms[b];
                v.w *= 5;  // the shift that picks the pair class out of an a-atom's fields
                s_b[tid] = v;
            }
            __syncthreads();
            loaded = tb;
        }
        const int a = ta * kSaxsTile + lane_atom, b_base = tb * kSaxsTile;
        const bool valid = a < h.n_atoms;
        const int4 me = valid ? atoms[a] : make_int4(0, 0, 0, 0);
        const uint32_t fields = saxs_pair_fields((uint32_t)me.w);
        const int j0 = max(half * (kSaxsTile / 2), h.first_b - b_base);
        const int j1 = min((half + 1) * (kSaxsTile / 2), h.n_atoms - b_base);
        // masked: the diagonal tile pair, where a lane may have no atom or its atom may not precede b.  Every other pair
        // has a full a-tile wholly in front of the b-tile: nothing to mask, and a pair beyond the last bin adds to the
        // spare word behind the histogram, so the loop's only branch is the rare exact path.
        auto walk = [&](auto masked) {
            auto pair = [&](const int4 &b, int j) {
                const int ix = me.x - b.x, iy = me.y - b.y, iz = me.z - b.z;
                const float fx = (float)ix, fy = (float)iy, fz = (float)iz;
                const float e = __builtin_amdgcn_sqrtf(__builtin_fmaf(fz, fz, __builtin_fmaf(fy, fy, fx * fx))) * inv_w;
                const float floor_e = floorf(e);
                uint32_t k = (uint32_t)floor_e;
                if (fabsf((e - floor_e) - 0.5f) > 0.5f - kSaxsEdge)  // within kSaxsEdge of a bin's edge: d^2 in 64 bits decides
                    k = saxs_bin(saxs_d2(saxs_axis(ix), saxs_axis(iy), saxs_axis(iz)), w, k);
                const uint32_t at = __umul24((fields >> b.w) & 31u, bins) + k;  // b.w: 5 x class
                if constexpr (decltype(masked)::value) {
                    if (valid && a < b_base + j) {
                        if (k < bins) __hip_atomic_fetch_add(&s_hist[at], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        else over = true;
                    }
                } else {
                    const bool in_range = k < bins;
                    over |= !in_range;
                    __hip_atomic_fetch_add(&s_hist[in_range ? at : (uint32_t)words], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            };
            int j = j0;
#pragma unroll 1
            for (; j + 4 <= j1; j += 4) {  // four broadcast reads in flight before the first add: an add may not pass a read
                const int4 b0 = s_b[j], b1 = s_b[j + 1], b2 = s_b[j + 2], b3 = s_b[j + 3];
                pair(b0, j);
                pair(b1, j + 1);
                pair(b2, j + 2);
                pair(b3, j + 3);
            }
#pragma unroll 1
            for (; j < j1; j++) pair(s_b[j], j);
        };
        if (ta == tb) walk(std::true_type());
        else walk(std::false_type());
        if (++ta > tb) ta = 0, tb++;
    }
    if (over) *h.overflow = 1;
    __syncthreads();
    uint32_t *row = h.counts + pose * (size_t)words;
    for (int i = tid; i < words; i += kSaxsThreads) {
        const uint32_t v = s_hist[i];
        if (v) __hip_atomic_fetch_add(&row[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ void __launch_bounds__(kSaxsDebyeThreads) saxs_debye(SaxsDebye d) {
    extern __shared__ uint32_t s_counts[];  // 21 x bins
    const int tid = threadIdx.x, words = kSaxsPairClasses * d.bins;
    const size_t pose = blockIdx.x;
    const uint32_t *row = d.counts + pose * (size_t)words;
    for (int i = tid; i < words; i += kSaxsDebyeThreads) s_counts[i] = row[i];
    __syncthreads();
#pragma unroll 1
    for (int j = tid; j < d.n_q; j += kSaxsDebyeThreads) {
        double G[kSaxsPairClasses];
#pragma unroll
        for (int c = 0; c < kSaxsPairClasses; c++) G[c] = 0.0;
#pragma unroll 1
        for (int k = 0; k < d.bins; k++) {
            const double s = d.sinc_t[(size_t)k * d.n_q + j];
#pragma unroll
            for (int c = 0; c < kSaxsPairClasses; c++) G[c] = G[c] + (double)s_counts[c * d.bins + k] * s;
        }
        double I = d.self[j];
#pragma unroll
        for (int c = 0; c < kSaxsPairClasses; c++) I = I + d.cross[(size_t)j * kSaxsPairClasses + c] * G[c];
        d.intensity[pose * (size_t)d.n_q + j] = I;
    }
}

}  // namespace

hipError_t launch_saxs_pose(const ComplexDevice &m, const SaxsDevice &d, const double *poses, size_t stride, size_t n, int first,
                            int count, int4 *out, size_t out_stride, int *overflow, hipStream_t stream) {
    if (n == 0 || count <= 0) return hipSuccess;
    if (n > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(saxs_pose, dim3((unsigned)((count + kSaxsPoseThreads - 1) / kSaxsPoseThreads), (unsigned)n), dim3(kSaxsPoseThreads), 0,
                       stream, m, d, poses, stride, first, count, out, out_stride, overflow);
    return hipGetLastError();
}

hipError_t launch_saxs_rows(const uint32_t *base, uint32_t *rows, size_t n, size_t row_words, hipStream_t stream) {
    if (n == 0 || row_words == 0) return hipSuccess;
    const size_t blocks = (n * row_words + 255) / 256;
    hipLaunchKernelGGL(saxs_rows, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream, base, rows, n, row_words);
    return hipGetLastError();
}

hipError_t launch_saxs_histogram(const SaxsHistogram &h, size_t n, hipStream_t stream) {
    if (n == 0 || saxs_tile_pairs(h.n_atoms, h.first_b) <= 0) return hipSuccess;
    if (n > 65535 || h.splits < 1 || h.bins < 1 || h.bins > kSaxsMaxBins) return hipErrorInvalidValue;
    const size_t lds = saxs_histogram_lds_bytes(h.bins);
    if (lds > 60 * 1024) {  // beyond the default limit of dynamic LDS
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&saxs_histogram), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(saxs_histogram, dim3((unsigned)h.splits, (unsigned)n), dim3(kSaxsThreads), lds, stream, h);
    return hipGetLastError();
}

hipError_t launch_saxs_debye(const SaxsDebye &d, size_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (d.bins < 1 || d.bins > kSaxsMaxBins || d.n_q < 1 || d.n_q > kSaxsMaxQ) return hipErrorInvalidValue;
    const size_t lds = saxs_histogram_lds_bytes(d.bins);
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&saxs_debye), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(saxs_debye, dim3((unsigned)n), dim3(kSaxsDebyeThreads), lds, stream, d);
    return hipGetLastError();
}

}  // namespace ld
