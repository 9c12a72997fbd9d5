// fcc.hip -- K3g: clustering a run's models by the fraction of common contacts (gfx950; lightdock_hip.h,
// "Clustering by common contacts").  Kernels and their launchers (kernels/fcc.hpp); the host side is fcc.cpp.
//   complex_pair_sets:    a workgroup a pose: the touching (receptor residue, ligand residue) pairs as a bitmap in the
//                         workgroup's slot, then their count or their keys in ascending order;
//   fcc_exclusive_scan:   counts -> CSR offsets, bitmap block counts -> ranks (one workgroup, a chunk at a time);
//   fcc_mark, fcc_rank_counts, fcc_rows: the union of all keys renumbered densely, every set as a bit row;
//   fcc_common:           the all-against-all c_ij = popcount(row_i & row_j), 64 x 64 tiles staged in LDS, 4 x 4 pairs a
//                         thread; neighbour bits (or c itself) leave the tile;
//   fcc_degrees, fcc_greedy: the greedy rounds inside ONE workgroup, counts updated by the rows of the poses that died;
//   fcc_consensus:        sum of the column frequencies of a set.
// No workgroup waits on another one inside a launch.
#include "kernels/fcc.hpp"

#include "kernels/complex_pose.hpp"

#include <algorithm>
#include <climits>
#include <cmath>

namespace ld {

namespace {

template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T v, int lane) {
    for (int s = 1; s < 64; s <<= 1) {
        const T o = __shfl_up(v, s);
        if (lane >= s) v += o;
    }
    return v;
}

// Every thread of the block calls it.  s_wave: kThreads / 64 words.  Returns the sum of v over the threads below this one.
template <int kThreads, typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T *s_wave, T *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T incl = wave_inclusive_scan(v, lane);
    __syncthreads();  // the words of the call before are read
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    T before = 0, all = 0;
    for (int w = 0; w < kThreads / 64; w++) {
        const T t = s_wave[w];
        if (w < wave) before += t;
        all += t;
    }
    *total = all;
    return before + incl - v;
}

// A word another wave of this workgroup ORed into with an atomic: read where the atomic ran.
__device__ __forceinline__ uint32_t load_word(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// --- pair sets --------------------------------------------------------------------------------------------------------
// complex_contacts's steps 1 to 3 (kernels/cluster.hip), with one difference: a surviving residue pair is always walked,
// and a touching one sets bit (r, l) of the slot's bitmap.  Step 4 reads the bitmap in order: a count, or the keys.

template <bool kFill>
__global__ void __launch_bounds__(kPairThreads, 8) complex_pair_sets(ComplexDevice m, ContactsDevice d, const double *poses,
                                                                     size_t stride, size_t n, uint32_t C2, int4 *atoms_ws,
                                                                     int *boxes_ws, uint32_t *pairs_ws, const uint32_t *offsets,
                                                                     uint32_t *counts, uint32_t *keys, int *overflow) {
    extern __shared__ uint32_t s_mem[];  // the scan's words, then the boxes if they fit
    constexpr int kWaves = kPairThreads / 64;
    uint32_t *s_wave = s_mem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lw = (d.n_lig_res + 31) >> 5;
    const size_t pair_words = (size_t)d.n_rec_res * lw;
    const int n_res = d.n_rec_res + d.n_lig_res, n_boxes = n_res + d.n_lig_grp;
    int4 *A = atoms_ws + (size_t)blockIdx.x * d.n_atoms;
    int *box = d.boxes_in_lds ? reinterpret_cast<int *>(s_mem + kWaves) : boxes_ws + (size_t)blockIdx.x * 6 * n_boxes;
    uint32_t *P = pairs_ws + (size_t)blockIdx.x * pair_words;
    const uint32_t *lig_start = d.res_start + d.n_rec_res;
    const int lig_grp = n_res, lig_res = d.n_rec_res;

    for (size_t pose = blockIdx.x; pose < n; pose += gridDim.x) {
        const double *row = poses + pose * stride;
        for (size_t w = tid; w < pair_words; w += kPairThreads) P[w] = 0;
        for (int r = tid; r < n_res; r += kPairThreads)
            store_box(box, n_boxes, r, Box{{INT_MAX, INT_MAX, INT_MAX}, {INT_MIN, INT_MIN, INT_MIN}});
        __syncthreads();
#pragma unroll 1
        for (int a = tid; a < d.n_atoms; a += kPairThreads) {
            int v[3];
            if (!posed_thousandths(m, row, (uint32_t)a, kComplexCoordBound, v)) *overflow = 1;
            const int r = (int)d.res_of_atom[a];
            for (int k = 0; k < 3; k++) {
                atomicMin(&box[k * n_boxes + r], v[k]);
                atomicMax(&box[(3 + k) * n_boxes + r], v[k]);
            }
            A[a] = make_int4(v[0], v[1], v[2], 0);
        }
        __syncthreads();
#pragma unroll 1
        for (int g = tid; g < d.n_lig_grp; g += kPairThreads) {
            const int r0 = lig_res + g * kResGroup, r1 = min(r0 + kResGroup, n_res);
            Box b = load_box(box, n_boxes, r0);
#pragma unroll 1
            for (int r = r0 + 1; r < r1; r++) {
                const Box o = load_box(box, n_boxes, r);
                for (int k = 0; k < 3; k++) b.lo[k] = min(b.lo[k], o.lo[k]), b.hi[k] = max(b.hi[k], o.hi[k]);
            }
            store_box(box, n_boxes, lig_grp + g, b);
        }
        __syncthreads();

        // all control flow below is uniform over the wave: the masks come from ballots
        Box whole{{INT_MAX, INT_MAX, INT_MAX}, {INT_MIN, INT_MIN, INT_MIN}};
        for (int g = lane; g < d.n_lig_grp; g += 64) {
            const Box o = load_box(box, n_boxes, lig_grp + g);
            for (int k = 0; k < 3; k++) whole.lo[k] = min(whole.lo[k], o.lo[k]), whole.hi[k] = max(whole.hi[k], o.hi[k]);
        }
        for (int step = 1; step < 64; step <<= 1)
            for (int k = 0; k < 3; k++) {
                whole.lo[k] = min(whole.lo[k], __shfl_xor(whole.lo[k], step));
                whole.hi[k] = max(whole.hi[k], __shfl_xor(whole.hi[k], step));
            }
        // receptor residue (64 i + lane) * waves + wave: a residue, and so a row of the bitmap, belongs to one wave
        for (int base = 0; base * kWaves < d.n_rec_res; base += 64) {
            const int mine = (base + lane) * kWaves + wave;
            const Box mb = load_box(box, n_boxes, min(mine, d.n_rec_res - 1));
            unsigned long long residues = __builtin_amdgcn_ballot_w64(mine < d.n_rec_res && boxes_within(mb, whole, C2));
            while (residues) {
                const int rr = (base + __ffsll(residues) - 1) * kWaves + wave;
                residues &= residues - 1;
                const Box rb = load_box(box, n_boxes, rr);
                const int a0 = (int)d.res_start[rr], a1 = (int)d.res_start[rr + 1];
                for (int lg0 = 0; lg0 < d.n_lig_grp; lg0 += 64) {
                    const int lg = lg0 + lane;
                    unsigned long long groups =
                        __builtin_amdgcn_ballot_w64(lg < d.n_lig_grp && boxes_within(rb, load_box(box, n_boxes, lig_grp + min(lg, d.n_lig_grp - 1)), C2));
                    while (groups) {
                        const int lgi = lg0 + __ffsll(groups) - 1;
                        groups &= groups - 1;
                        const int l = lgi * kResGroup + lane;  // the first kResGroup lanes: a ligand residue each
                        unsigned long long pairs = __builtin_amdgcn_ballot_w64(
                            lane < kResGroup && l < d.n_lig_res && boxes_within(rb, load_box(box, n_boxes, lig_res + min(l, d.n_lig_res - 1)), C2));
                        while (pairs) {
                            const int ll = lgi * kResGroup + __ffsll(pairs) - 1;
                            pairs &= pairs - 1;
                            const int b0 = (int)lig_start[ll], b1 = (int)lig_start[ll + 1];
                            bool hit = false;
                            for (int ta = a0; ta < a1 && !hit; ta += 8)
                                for (int tb = b0; tb < b1 && !hit; tb += 8) {
                                    const int a = ta + (lane >> 3), b = tb + (lane & 7);
                                    hit = __builtin_amdgcn_ballot_w64(a < a1 && b < b1 && in_contact(A[min(a, a1 - 1)], A[min(b, b1 - 1)], C2)) != 0;
                                }
                            if (hit && lane == 0) atomicOr(&P[(size_t)rr * lw + (ll >> 5)], 1u << (ll & 31));
                        }
                    }
                }
            }
        }
        __syncthreads();
        if (!kFill) {
            uint32_t mine = 0;
            for (size_t w = tid; w < pair_words; w += kPairThreads) mine += (uint32_t)__popc(load_word(&P[w]));
            uint32_t all;
            (void)block_exclusive_scan<kPairThreads>(mine, s_wave, &all);
            if (tid == 0) counts[pose] = all;
        } else {
            // in order: a word a thread, the keys of a chunk of words behind those of the chunks before it
            size_t at = offsets[pose];
            for (size_t w0 = 0; w0 < pair_words; w0 += kPairThreads) {
                const size_t w = w0 + tid;
                uint32_t word = w < pair_words ? load_word(&P[w]) : 0;
                uint32_t all;
                size_t out = at + block_exclusive_scan<kPairThreads>((uint32_t)__popc(word), s_wave, &all);
                const uint32_t r = (uint32_t)(w / lw), l0 = (uint32_t)(w % lw) * 32;
                while (word) {
                    const uint32_t l = l0 + (uint32_t)__ffs(word) - 1;
                    word &= word - 1;
                    keys[out++] = r * (uint32_t)d.n_lig_res + l;
                }
                at += all;
            }
        }
        __syncthreads();  // the slot is reused by the next pose
    }
}

__global__ void __launch_bounds__(kFccScanThreads) fcc_exclusive_scan(const uint32_t *in, size_t n, uint32_t *out,
                                                                      unsigned long long *total) {
    __shared__ unsigned long long s_wave[kFccScanThreads / 64];
    unsigned long long running = 0;
    for (size_t i0 = 0; i0 < n; i0 += kFccScanThreads) {
        const size_t i = i0 + threadIdx.x;
        const unsigned long long v = i < n ? in[i] : 0;
        unsigned long long all;
        const unsigned long long before = block_exclusive_scan<kFccScanThreads>(v, s_wave, &all);
        if (i < n) out[i] = (uint32_t)(running + before);
        running += all;
    }
    if (threadIdx.x == 0) {
        out[n] = (uint32_t)running;
        *total = running;
    }
}

// --- the union of all keys, renumbered densely; every set as a bit row --------------------------------------------------

__global__ void __launch_bounds__(256) fcc_mark(const uint32_t *keys, size_t total, uint32_t key_lo, uint32_t *bitmap) {
    for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (size_t)gridDim.x * blockDim.x) {
        const uint32_t k = keys[x] - key_lo;
        atomicOr(&bitmap[k >> 5], 1u << (k & 31));
    }
}

__global__ void __launch_bounds__(256) fcc_rank_counts(const uint32_t *bitmap, size_t n_rank, uint32_t *rank) {
    for (size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x; b < n_rank; b += (size_t)gridDim.x * blockDim.x) {
        uint32_t count = 0;
        for (int w = 0; w < kFccRankWords; w++) count += (uint32_t)__popc(bitmap[b * kFccRankWords + w]);
        rank[b] = count;
    }
}

__global__ void __launch_bounds__(256) fcc_rows(const uint32_t *offsets, const uint32_t *keys, size_t n, const uint32_t *row_of,
                                                uint32_t key_lo, const uint32_t *bitmap, const uint32_t *rank, size_t W,
                                                uint32_t *rows, uint32_t *cols, uint32_t *freq, uint32_t *sizes) {
    const int lane = threadIdx.x & 63;
    const size_t waves = (size_t)gridDim.x * (blockDim.x >> 6);
    for (size_t i = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < n; i += waves) {
        const size_t row = row_of ? row_of[i] : i;
        const size_t b = offsets[i], e = offsets[i + 1];
        if (lane == 0) sizes[row] = (uint32_t)(e - b);
        for (size_t x = b + lane; x < e; x += 64) {
            const uint32_t k = keys[x] - key_lo;
            const size_t word = k >> 5, first = word / kFccRankWords * kFccRankWords;
            uint32_t col = rank[word / kFccRankWords];
            for (size_t w = first; w < word; w++) col += (uint32_t)__popc(bitmap[w]);
            col += (uint32_t)__popc(bitmap[word] & ((1u << (k & 31)) - 1u));
            cols[x] = col;
            atomicOr(&rows[row * W + (col >> 5)], 1u << (col & 31));
            atomicAdd(&freq[col], 1u);
        }
    }
}

// --- common contacts ----------------------------------------------------------------------------------------------------
// Tile (bi, bj), bj >= bi: rows I0 .. I0 + 63 against rows J0 .. J0 + 63.  A chunk of kFccChunkWords words of both row
// sets is staged word-major (s[k][row], kFccLdsStride words a k) so that a thread reads its four rows of either side with
// one 16-byte load: the A load is one address for the 16 lanes that share ty (a broadcast), the B load 16 consecutive
// quads.  32 v_and + 32 v_bcnt (with its add) against two LDS loads a word: the VALU is the limit, not LDS.

template <bool kBits>
__global__ void __launch_bounds__(kFccCommonThreads) fcc_common(const uint32_t *rows, size_t W, size_t n, const uint32_t *sizes,
                                                                uint32_t T, uint32_t *nbr, uint32_t *common) {
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj < bi) return;
    __shared__ __attribute__((aligned(16))) uint32_t sA[kFccChunkWords * kFccLdsStride];
    __shared__ __attribute__((aligned(16))) uint32_t sB[kFccChunkWords * kFccLdsStride];
    __shared__ uint32_t s_bits[kFccTile * 2], s_mirror[kFccTile * 2];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const size_t I0 = (size_t)bi * kFccTile, J0 = (size_t)bj * kFccTile;
    if (kBits && tid < kFccTile * 2) s_bits[tid] = 0, s_mirror[tid] = 0;  // the chunk loop's barriers come before their use

    uint32_t acc[4][4] = {};
    const int k = tid & 31, r0 = tid >> 5;
    for (size_t k0 = 0; k0 < W; k0 += kFccChunkWords) {
        const bool k_in = k0 + k < W;
#pragma unroll
        for (int p = 0; p < kFccTile / 8; p++) {
            const int r = r0 + 8 * p;
            const size_t gi = I0 + r, gj = J0 + r;
            sA[k * kFccLdsStride + r] = (k_in && gi < n) ? rows[gi * W + k0 + k] : 0u;
            sB[k * kFccLdsStride + r] = (k_in && gj < n) ? rows[gj * W + k0 + k] : 0u;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < kFccChunkWords; kk++) {  // words beyond W are staged as zeros
            const uint4 a = *reinterpret_cast<const uint4 *>(&sA[kk * kFccLdsStride + 4 * ty]);
            const uint4 b = *reinterpret_cast<const uint4 *>(&sB[kk * kFccLdsStride + 4 * tx]);
            const uint32_t av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int x = 0; x < 4; x++)
#pragma unroll
                for (int y = 0; y < 4; y++) acc[x][y] += (uint32_t)__popc(av[x] & bv[y]);
        }
        __syncthreads();
    }

    if (kBits) {
#pragma unroll
        for (int x = 0; x < 4; x++) {
            const int ri = 4 * ty + x;
            const size_t gi = I0 + ri;
            if (gi >= n) continue;
            const uint32_t si = sizes[gi];
#pragma unroll
            for (int y = 0; y < 4; y++) {
                const int rj = 4 * tx + y;
                const size_t gj = J0 + rj;
                if (gj >= n || gi == gj || !fcc_neighbours(acc[x][y], si, sizes[gj], T)) continue;
                atomicOr(&s_bits[ri * 2 + (rj >> 5)], 1u << (rj & 31));
                atomicOr(&s_mirror[rj * 2 + (ri >> 5)], 1u << (ri & 31));
            }
        }
        __syncthreads();
        const size_t NW = (n + 31) / 32;
        if (tid < kFccTile * 2) {
            const int r = tid >> 1, h = tid & 1;
            const size_t gi = I0 + r, wj = J0 / 32 + h;
            if (gi < n && wj < NW) nbr[gi * NW + wj] = s_bits[tid];
            const size_t gj = J0 + r, wi = I0 / 32 + h;
            if (bi != bj && gj < n && wi < NW) nbr[gj * NW + wi] = s_mirror[tid];
        }
    } else {
#pragma unroll
        for (int x = 0; x < 4; x++)
#pragma unroll
            for (int y = 0; y < 4; y++) {
                const size_t gi = I0 + 4 * ty + x, gj = J0 + 4 * tx + y;
                if (gi >= n || gj >= n) continue;
                common[gi * n + gj] = acc[x][y];
                if (bi != bj) common[gj * n + gi] = acc[x][y];
            }
    }
}

__global__ void __launch_bounds__(256) fcc_degrees(const uint32_t *nbr, size_t n, int *deg) {
    const int lane = threadIdx.x & 63;
    const size_t NW = (n + 31) / 32, waves = (size_t)gridDim.x * (blockDim.x >> 6);
    for (size_t i = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < n; i += waves) {
        int count = 0;
        for (size_t w = lane; w < NW; w += 64) count += __popc(nbr[i * NW + w]);
        for (int step = 1; step < 64; step <<= 1) count += __shfl_xor(count, step);
        if (lane == 0) deg[i] = 1 + count;
    }
}

// --- the greedy rounds --------------------------------------------------------------------------------------------------
// One workgroup runs every round, so the barrier of a workgroup is all the synchronisation there is.  A round: the alive row
// with the largest (deg, -row); its alive neighbours and itself die as the next cluster; every row that died takes 1 off
// the count of each of its alive neighbours.  Over all rounds every row of the neighbour bits is read once as a centre at
// most and once as a member at most.  When the largest count is 1 no alive row has an alive neighbour: the rest are
// clusters of one in row order, numbered by one scan.

__global__ void __launch_bounds__(kFccGreedyThreads) fcc_greedy(const uint32_t *nbr, size_t n, int *deg, uint32_t min_size,
                                                                int *members, int32_t *cluster_of, int32_t *centres,
                                                                FccStatus *status) {
    constexpr int kWaves = kFccGreedyThreads / 64;
    __shared__ uint32_t s_alive[kFccMaxSets / 32];
    __shared__ unsigned long long s_best[kWaves];
    __shared__ uint32_t s_wave[kWaves];
    __shared__ int s_count;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t NW = (n + 31) / 32;
    for (size_t w = tid; w < NW; w += kFccGreedyThreads)
        s_alive[w] = (w + 1) * 32 <= n ? 0xffffffffu : (1u << (n & 31)) - 1u;
    for (size_t i = tid; i < n; i += kFccGreedyThreads) cluster_of[i] = -1, centres[i] = -1;
    __syncthreads();

    uint32_t cid = 0, rounds = 0;
    for (;;) {
        unsigned long long best = 0;
        for (size_t i = tid; i < n; i += kFccGreedyThreads)
            if (s_alive[i >> 5] >> (i & 31) & 1u) {
                const unsigned long long d = (uint32_t)__hip_atomic_load(&deg[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned long long key = d << 32 | (0xffffffffu - (uint32_t)i);
                best = key > best ? key : best;
            }
        for (int step = 1; step < 64; step <<= 1) {
            const unsigned long long o = __shfl_xor(best, step);
            best = o > best ? o : best;
        }
        __syncthreads();  // s_best of the round before is read
        if (lane == 0) s_best[wave] = best;
        __syncthreads();
        best = 0;
        for (int w = 0; w < kWaves; w++) best = s_best[w] > best ? s_best[w] : best;
        if (best == 0) break;  // nobody is alive: a count is 1 at least
        const uint32_t d = (uint32_t)(best >> 32), centre = 0xffffffffu - (uint32_t)best;
        if (d < min_size) break;
        if (d == 1) {
            for (size_t i0 = 0; i0 < n; i0 += kFccGreedyThreads) {
                const size_t i = i0 + tid;
                const uint32_t alive = i < n ? s_alive[i >> 5] >> (i & 31) & 1u : 0u;
                uint32_t all;
                const uint32_t mine = cid + block_exclusive_scan<kFccGreedyThreads>(alive, s_wave, &all);
                if (alive) cluster_of[i] = (int32_t)mine, centres[mine] = (int32_t)i;
                cid += all;
            }
            break;
        }
        if (tid == 0) s_count = 0;
        __syncthreads();
        for (size_t w = tid; w < NW; w += kFccGreedyThreads) {
            uint32_t bits = nbr[(size_t)centre * NW + w] & s_alive[w];
            if (w == centre >> 5) bits |= 1u << (centre & 31);
            s_alive[w] &= ~bits;
            while (bits) {
                const uint32_t i = (uint32_t)w * 32 + (uint32_t)__ffs(bits) - 1;
                bits &= bits - 1;
                members[atomicAdd(&s_count, 1)] = (int)i;
                cluster_of[i] = (int32_t)cid;
            }
        }
        if (tid == 0) centres[cid] = (int32_t)centre;
        __syncthreads();
        const size_t work = (size_t)s_count * NW;
        for (size_t x = tid; x < work; x += kFccGreedyThreads) {
            const size_t w = x % NW;
            uint32_t bits = nbr[(size_t)members[x / NW] * NW + w] & s_alive[w];
            while (bits) {
                atomicSub(&deg[w * 32 + (uint32_t)__ffs(bits) - 1], 1);
                bits &= bits - 1;
            }
        }
        __syncthreads();
        cid++;
        rounds++;
    }
    if (tid == 0) status->n_clusters = cid, status->rounds = rounds;
}

__global__ void __launch_bounds__(256) fcc_consensus(const uint32_t *offsets, const uint32_t *cols, const uint32_t *freq, size_t n,
                                                     unsigned long long *consensus) {
    const int lane = threadIdx.x & 63;
    const size_t waves = (size_t)gridDim.x * (blockDim.x >> 6);
    for (size_t i = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < n; i += waves) {
        unsigned long long sum = 0;
        for (size_t x = (size_t)offsets[i] + lane; x < offsets[i + 1]; x += 64) sum += freq[cols[x]];
        for (int step = 1; step < 64; step <<= 1) sum += __shfl_xor(sum, step);
        if (lane == 0) consensus[i] = sum;
    }
}

unsigned grid_of(size_t items, size_t per_block) {
    return (unsigned)std::max<size_t>(1, std::min<size_t>((items + per_block - 1) / per_block, 8192));
}

}  // namespace

hipError_t launch_complex_pair_sets(const ComplexDevice &m, const ContactsDevice &d, const double *poses, size_t stride, size_t n,
                                    uint32_t C2, size_t slots, int4 *atoms_ws, int *boxes_ws, uint32_t *pairs_ws,
                                    const uint32_t *offsets, uint32_t *counts, uint32_t *keys, int *overflow, hipStream_t stream) {
    const size_t lds = (kPairThreads / 64) * sizeof(uint32_t) + (d.boxes_in_lds ? d.box_bytes() : 0);
    if (offsets)
        hipLaunchKernelGGL(complex_pair_sets<true>, dim3((unsigned)slots), dim3(kPairThreads), lds, stream, m, d, poses, stride, n, C2,
                           atoms_ws, boxes_ws, pairs_ws, offsets, counts, keys, overflow);
    else
        hipLaunchKernelGGL(complex_pair_sets<false>, dim3((unsigned)slots), dim3(kPairThreads), lds, stream, m, d, poses, stride, n, C2,
                           atoms_ws, boxes_ws, pairs_ws, offsets, counts, keys, overflow);
    return hipGetLastError();
}

hipError_t launch_fcc_exclusive_scan(const uint32_t *in, size_t n, uint32_t *out, unsigned long long *total, hipStream_t stream) {
    hipLaunchKernelGGL(fcc_exclusive_scan, dim3(1), dim3(kFccScanThreads), 0, stream, in, n, out, total);
    return hipGetLastError();
}

hipError_t launch_fcc_mark(const uint32_t *keys, size_t total, uint32_t key_lo, uint32_t *bitmap, hipStream_t stream) {
    hipLaunchKernelGGL(fcc_mark, dim3(grid_of(total, 256)), dim3(256), 0, stream, keys, total, key_lo, bitmap);
    return hipGetLastError();
}

hipError_t launch_fcc_rank_counts(const uint32_t *bitmap, size_t n_rank, uint32_t *rank, hipStream_t stream) {
    hipLaunchKernelGGL(fcc_rank_counts, dim3(grid_of(n_rank, 256)), dim3(256), 0, stream, bitmap, n_rank, rank);
    return hipGetLastError();
}

hipError_t launch_fcc_rows(const uint32_t *offsets, const uint32_t *keys, size_t n, const uint32_t *row_of, uint32_t key_lo,
                           const uint32_t *bitmap, const uint32_t *rank, size_t W, uint32_t *rows, uint32_t *cols,
                           uint32_t *freq, uint32_t *sizes, hipStream_t stream) {
    hipLaunchKernelGGL(fcc_rows, dim3(grid_of(n, 4)), dim3(256), 0, stream, offsets, keys, n, row_of, key_lo, bitmap, rank, W, rows,
                       cols, freq, sizes);
    return hipGetLastError();
}

hipError_t launch_fcc_common(const uint32_t *rows, size_t W, size_t n, const uint32_t *sizes, uint32_t T, uint32_t *nbr,
                             uint32_t *common, hipStream_t stream) {
    if ((nbr == nullptr) == (common == nullptr) || n > kFccMaxSets || W == 0) return hipErrorInvalidValue;
    const unsigned tiles = (unsigned)((n + kFccTile - 1) / kFccTile);
    if (nbr)
        hipLaunchKernelGGL(fcc_common<true>, dim3(tiles, tiles), dim3(kFccCommonThreads), 0, stream, rows, W, n, sizes, T, nbr, common);
    else
        hipLaunchKernelGGL(fcc_common<false>, dim3(tiles, tiles), dim3(kFccCommonThreads), 0, stream, rows, W, n, sizes, T, nbr, common);
    return hipGetLastError();
}

hipError_t launch_fcc_degrees(const uint32_t *nbr, size_t n, int *deg, hipStream_t stream) {
    hipLaunchKernelGGL(fcc_degrees, dim3(grid_of(n, 4)), dim3(256), 0, stream, nbr, n, deg);
    return hipGetLastError();
}

hipError_t launch_fcc_greedy(const uint32_t *nbr, size_t n, int *deg, uint32_t min_size, int *members, int32_t *cluster_of,
                             int32_t *centres, FccStatus *status, hipStream_t stream) {
    if (n > kFccMaxSets) return hipErrorInvalidValue;  // the alive bits are LDS
    hipLaunchKernelGGL(fcc_greedy, dim3(1), dim3(kFccGreedyThreads), 0, stream, nbr, n, deg, min_size, members, cluster_of, centres,
                       status);
    return hipGetLastError();
}

hipError_t launch_fcc_consensus(const uint32_t *offsets, const uint32_t *cols, const uint32_t *freq, size_t n,
                                unsigned long long *consensus, hipStream_t stream) {
    hipLaunchKernelGGL(fcc_consensus, dim3(grid_of(n, 4)), dim3(256), 0, stream, offsets, cols, freq, n, consensus);
    return hipGetLastError();
}

}  // namespace ld
