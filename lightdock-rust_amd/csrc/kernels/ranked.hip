// ranked.hip -- K3e: BSAS over ONE ranked list of up to about a million poses, in several workgroups (gfx950; DESIGN §5
// K3e; lightdock_hip.h, "Clustering a ranked list").  Kernels and their launchers (kernels/ranked.hpp); the host side is
// Complex::cluster_ranked in complex.cpp, which sorts, uploads the pose rows in sorted order and loops over the rounds.
//   ranked_begin:  state = -1, the status words, and s_max: the largest f64 S for which within_cutoff (the predicate of
//                  complex_bsas, kernels/complex_pose.hpp) holds, by bisection over the bit patterns of the non-negative
//                  doubles.  within_cutoff is non-decreasing in S, so `S <= s_max` IS within_cutoff(S), for every S;
//   ranked_pose:   every pose's walked atoms once, as thousandths, position fastest;
//   ranked_pick:   one workgroup.  The first 64 unresolved positions from the cursor are the candidates; their pairs are
//                  decided in parallel, a granule of 32 atoms at a time staged in LDS; then one thread walks the 64-bit
//                  masks: candidate k leads iff none of the leaders before it is near it, else it joins the first of them;
//   ranked_sweep:  a lane a position behind the candidates.  An unresolved lane holds its first granule in registers and
//                  tests it against every leader of the round (LDS, the same address for all lanes); the survivors are
//                  walked further, leader by leader in creation order, with the early exit; it joins the first that holds.
// After a round's sweep every unresolved position is beyond the cutoff of every leader so far, so the candidates of the
// next round need only each other: the result is the sequential loop's.  S is a sum of squares of exact integers in f64
// (fma), exact and order-free below 2^53, which is complex_bsas's premise too; any atom order gives the same decisions,
// and the ligand's atoms, which move most, are walked first.  No kernel waits on another workgroup.
#include "kernels/ranked.hpp"

#include "kernels/complex_pose.hpp"

#include <algorithm>
#include <cfloat>
#include <climits>

namespace ld {

namespace {

constexpr int kPickWaves = kRankedPickThreads / 64;
constexpr int kPickStride = kRankedRows + 1;  // words a candidate in LDS: an odd stride spreads the lanes over the banks

// S + (a - b)^2.  |a - b| < 2^32 exactly, whatever the two int32 are.
__device__ __forceinline__ double add_term(double S, int a, int b) {
    const double d = (double)((uint32_t)max(a, b) - (uint32_t)min(a, b));
    return fma(d, d, S);
}

__global__ void __launch_bounds__(kPoseThreads) ranked_begin(RankedLaunch r, double cutoff, double n_atoms) {
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < (size_t)r.n; p += (size_t)gridDim.x * blockDim.x)
        r.state[p] = -1;
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    RankedStatus *st = r.status;
    double s_max = -1.0;
    if (within_cutoff(0.0, n_atoms, cutoff)) {
        unsigned long long lo = 0, hi = (unsigned long long)__double_as_longlong(DBL_MAX);  // lo holds, hi does not
        if (within_cutoff(DBL_MAX, n_atoms, cutoff)) lo = hi;
        while (hi - lo > 1) {
            const unsigned long long mid = lo + (hi - lo) / 2;
            if (within_cutoff(__longlong_as_double((long long)mid), n_atoms, cutoff))
                lo = mid;
            else
                hi = mid;
        }
        s_max = __longlong_as_double((long long)lo);
    }
    st->s_max = s_max;
    st->cursor = 0;
    st->n_clusters = 0;
    st->n_candidates = 0;
    st->n_leaders = 0;
    st->overflow = 0;
    st->rounds = 0;
}

// As complex_pose_thousandths with one swarm of n glowworms, over the walk list.
__global__ void __launch_bounds__(kPoseThreads) ranked_pose(ComplexDevice m, const double *poses, size_t stride, int n,
                                                            const uint32_t *walk, int n_walk, int32_t *ws, RankedStatus *status) {
    const size_t total = (size_t)n_walk * n;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t a = t / n;
        const size_t p = t - a * n;
        int v[3];
        if (!posed_thousandths(m, poses + p * stride, walk[a], INT_MAX, v)) status->overflow = 1;
        for (int k = 0; k < 3; k++) ws[(a * 3 + k) * n + p] = v[k];
    }
}

__global__ void __launch_bounds__(kRankedPickThreads) ranked_pick(RankedLaunch r, const int32_t *__restrict__ ws) {
    __shared__ int s_cand[kRankedBlock];
    __shared__ int s_lid[kRankedBlock];
    __shared__ unsigned long long s_near[kRankedBlock];  // bit j of word k: candidates j < k are within the cutoff
    __shared__ int s_open[kPickWaves];
    __shared__ int32_t s_xyz[kRankedBlock * kPickStride];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    RankedStatus *st = r.status;
    const int cursor = st->cursor;
    const double s_max = st->s_max;
    const size_t n = (size_t)r.n;

    // the candidates: the first kRankedBlock unresolved positions from the cursor (every thread keeps the same count)
    int found = 0;
    for (int base = cursor; base < r.n && found < kRankedBlock; base += kRankedPickThreads) {
        const int p = base + tid;
        const bool open = p < r.n && r.state[p] == -1;
        const unsigned long long b = __ballot(open);
        if (lane == 0) s_open[wave] = __popcll(b);
        __syncthreads();
        int before = found, total = found;
        for (int w = 0; w < kPickWaves; w++) {
            const int c = s_open[w];
            if (w < wave) before += c;
            total += c;
        }
        if (open) {
            const int k = before + __popcll(b & ((1ull << lane) - 1));
            if (k < kRankedBlock) s_cand[k] = p;
        }
        found = total;
        __syncthreads();
    }
    const int nc = min(found, kRankedBlock);
    if (tid < kRankedBlock) s_near[tid] = 0;

    // the pairs (j, k), j < k, in the order k (k - 1) / 2 + j: at most 2016, two a thread
    const int n_pairs = nc * (nc - 1) / 2;
    int pj[2], pk[2];
    bool live[2];
    double S[2] = {0.0, 0.0};
    for (int i = 0; i < 2; i++) {
        const int p = tid + i * kRankedPickThreads;
        int k = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)p)) * 0.5f);
        while (k * (k - 1) / 2 > p) k--;
        while ((k + 1) * k / 2 <= p) k++;
        pk[i] = k;
        pj[i] = p - k * (k - 1) / 2;
        live[i] = p < n_pairs;
    }
    for (int a0 = 0; a0 < r.n_walk; a0 += kRankedGranule) {
        if (!__syncthreads_or(live[0] || live[1])) break;  // also: the last granule's readers are done, s_near is cleared
        const int rows = 3 * min(kRankedGranule, r.n_walk - a0);
        for (int idx = tid; idx < nc * rows; idx += kRankedPickThreads) {
            const int row = idx / nc, c = idx - row * nc;
            s_xyz[c * kPickStride + row] = ws[(size_t)(3 * a0 + row) * n + s_cand[c]];
        }
        __syncthreads();
        for (int i = 0; i < 2; i++) {
            if (!live[i]) continue;
            const int32_t *a = s_xyz + pj[i] * kPickStride, *b = s_xyz + pk[i] * kPickStride;
            double s = S[i];
            for (int row = 0; row < rows; row++) s = add_term(s, a[row], b[row]);
            S[i] = s;
            live[i] = s <= s_max;  // a partial sum that fails, fails
        }
    }
    __syncthreads();
    for (int i = 0; i < 2; i++)
        if (live[i]) atomicOr(&s_near[pk[i]], 1ull << pj[i]);
    __syncthreads();

    if (tid == 0) {
        const int first = st->n_clusters;
        unsigned long long leaders = 0;
        int count = 0;
        for (int k = 0; k < nc; k++) {
            const unsigned long long m = s_near[k] & leaders;  // an absorbed candidate leads nobody
            const int p = s_cand[k];
            if (m == 0) {
                leaders |= 1ull << k;
                s_lid[k] = count;
                st->leaders[count] = p;
                r.reps[first + count] = p;
                r.state[p] = first + count;
                count++;
            } else {
                r.state[p] = first + s_lid[__ffsll(m) - 1];
            }
        }
        st->n_clusters = first + count;
        st->n_leaders = count;
        st->n_candidates = nc;
        st->cursor = nc ? s_cand[nc - 1] + 1 : r.n;
        st->rounds += nc ? 1 : 0;
    }
}

// base[offset / 4] as a uniform 64-bit base and a 32-bit byte offset a lane (n x 4 B is below 2^32: kRankedWorkspaceBytes),
// so that a row's address costs no registers.
__device__ __forceinline__ int32_t at_bytes(const int32_t *base, uint32_t offset) {
    return *reinterpret_cast<const int32_t *>(reinterpret_cast<const char *>(base) + offset);
}

// The sum over a lane's first granule against a leader's (LDS, one address for all lanes).  Three chains, one a
// coordinate: every partial sum is an exact integer below 2^53, so their sum is the one chain's.
__device__ __forceinline__ double first_granule(const int32_t (&own)[kRankedRows], const int32_t *q) {
    double s[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int row = 0; row < kRankedRows; row++) {
        s[row % 3] = add_term(s[row % 3], own[row], q[row]);
    }
    return s[0] + s[1] + s[2];
}

__global__ void __launch_bounds__(kRankedSweepThreads, 2) ranked_sweep(RankedLaunch r, const int32_t *__restrict__ ws, int from) {
    __shared__ __attribute__((aligned(16))) int32_t s_lead[kRankedBlock * kRankedRows];  // [leader][row], 0 beyond the granule
    const RankedStatus *st = r.status;
    const int n_leaders = st->n_leaders, start = st->cursor;
    const int tid = threadIdx.x;
    const int block0 = from + (int)blockIdx.x * kRankedSweepThreads;
    if (n_leaders == 0 || block0 + kRankedSweepThreads <= start) return;  // the whole workgroup
    const double s_max = st->s_max;
    const size_t n = (size_t)r.n;
    const int g_rows = 3 * min(kRankedGranule, r.n_walk);
    for (int idx = tid; idx < n_leaders * kRankedRows; idx += kRankedSweepThreads) {
        const int l = idx / kRankedRows, row = idx - l * kRankedRows;
        s_lead[idx] = row < g_rows ? ws[(size_t)row * n + st->leaders[l]] : 0;
    }
    __syncthreads();

    const int pos = block0 + tid;
    const bool active = pos >= start && pos < r.n && r.state[pos] == -1;
    if (!__ballot(active)) return;  // no barrier follows
    // the lane's own first granule, in registers (every index below is a constant once unrolled)
    // (straight-line loads, a uniform row base and the lane's 32-bit offset: an idle lane reads a valid position, rows
    // beyond the granule repeat its last row; both are zeroed)
    const uint32_t at = (uint32_t)min(pos, r.n - 1);
    int32_t own[kRankedRows];
#pragma unroll
    for (int row = 0; row < kRankedRows; row++) {
        const int32_t v = at_bytes(ws + (size_t)min(row, g_rows - 1) * n, 4u * at);
        own[row] = row < g_rows ? v : 0;
    }

    // leader by leader in creation order, the whole wave together (a leader's coordinates are one address for all
    // lanes): the first granule from registers and LDS; the lanes that survive it are walked further with the early
    // exit; a lane joins the first leader that holds to the end
    int joined = -1;
#pragma unroll 1
    for (int l = 0; l < n_leaders && __ballot(active && joined < 0); l++) {
        double s = first_granule(own, s_lead + l * kRankedRows);
        bool walk = active && joined < 0 && s <= s_max;
        if (r.n_walk > kRankedGranule && __ballot(walk)) {
            const uint32_t lp = (uint32_t)__builtin_amdgcn_readfirstlane(st->leaders[l]);
#pragma unroll 1
            for (int a0 = kRankedGranule; a0 < r.n_walk && __ballot(walk); a0 += kRankedGranule) {
                const int rows = 3 * min(kRankedGranule, r.n_walk - a0);
                if (walk) {
                    for (int row = 0; row < rows; row++) {
                        const int32_t *base = ws + (size_t)(3 * a0 + row) * n;
                        s = add_term(s, at_bytes(base, 4u * at), base[lp]);
                    }
                    walk = s <= s_max;
                }
            }
        }
        if (walk) joined = l;
    }
    if (joined >= 0) r.state[pos] = st->n_clusters - n_leaders + joined;
}

unsigned ranked_grid(size_t total, int threads) {
    const size_t blocks = (total + threads - 1) / threads;
    return (unsigned)std::max<size_t>(1, std::min<size_t>(blocks, 8192));
}

}  // namespace

hipError_t launch_ranked_pose(const ComplexDevice &m, const double *poses, size_t stride, int n, const uint32_t *walk, int n_walk,
                              int32_t *ws, RankedStatus *status, hipStream_t stream) {
    hipLaunchKernelGGL(ranked_pose, dim3(ranked_grid((size_t)n * n_walk, kPoseThreads)), dim3(kPoseThreads), 0, stream, m, poses,
                       stride, n, walk, n_walk, ws, status);
    return hipGetLastError();
}

hipError_t launch_ranked_begin(const RankedLaunch &r, double cutoff, double n_atoms, hipStream_t stream) {
    hipLaunchKernelGGL(ranked_begin, dim3(ranked_grid((size_t)r.n, kPoseThreads)), dim3(kPoseThreads), 0, stream, r, cutoff, n_atoms);
    return hipGetLastError();
}

hipError_t launch_ranked_pick(const RankedLaunch &r, const int32_t *ws, hipStream_t stream) {
    hipLaunchKernelGGL(ranked_pick, dim3(1), dim3(kRankedPickThreads), 0, stream, r, ws);
    return hipGetLastError();
}

hipError_t launch_ranked_sweep(const RankedLaunch &r, const int32_t *ws, int from, hipStream_t stream) {
    if (from >= r.n) return hipSuccess;  // nothing behind the candidates
    const unsigned blocks = (unsigned)(((size_t)(r.n - from) + kRankedSweepThreads - 1) / kRankedSweepThreads);
    hipLaunchKernelGGL(ranked_sweep, dim3(blocks), dim3(kRankedSweepThreads), 0, stream, r, ws, from);
    return hipGetLastError();
}

}  // namespace ld
