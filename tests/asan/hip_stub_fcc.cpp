// hip_stub_fcc.cpp -- TEST INFRASTRUCTURE for the sanitizer build of the host side (`make asan`, `make asan-fcc`): the
// launches of kernels/fcc.hpp, beside tests/asan/hip_stub.cpp which stands in for the HIP runtime and every other kernel.
// Device memory is host memory there, so ASan checks every extent below against what fcc.cpp allocated.  The launches do
// their kernels' work in plain C++ from the rule both sides share (fcc_neighbours is host code too): posing and rounding
// by the kernel's own kernels/complex_rule.hpp, every atom pair of every residue pair -- no boxes, no bitmap of a slot --
// and sets compared key by key, not as bit rows' words, so a disagreement with the kernels' structure would show.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "kernels/complex_rule.hpp"
#include "kernels/fcc.hpp"
#include "stub_access.hpp"

namespace ld {

hipError_t launch_complex_pair_sets(const ComplexDevice &m, const ContactsDevice &d, const double *poses, size_t stride, size_t n,
                                    uint32_t C2, size_t slots, int4 *atoms_ws, int *boxes_ws, uint32_t *pairs_ws,
                                    const uint32_t *offsets, uint32_t *counts, uint32_t *keys, int *overflow, hipStream_t) {
    const size_t lw = ((size_t)d.n_lig_res + 31) >> 5, n_boxes = (size_t)d.n_rec_res + d.n_lig_res + d.n_lig_grp;
    if (slots < 1 || slots > (size_t)kPairSlots || slots > n) return hipErrorInvalidValue;
    if ((kPairThreads / 64) * sizeof(uint32_t) + (d.boxes_in_lds ? n_boxes * 6 * sizeof(int) : 0) > 160 * 1024) return hipErrorInvalidValue;
    if ((uint64_t)d.n_rec_res * (uint64_t)d.n_lig_res >= (uint64_t(1) << 32) || d.n_atoms != m.n_rec + m.n_lig) return hipErrorInvalidValue;
    peek_complex(m, poses, stride, n);
    peek(d.res_start, (size_t)d.n_rec_res + d.n_lig_res + 1);
    peek(d.res_of_atom, (size_t)d.n_atoms);
    touch(atoms_ws, slots * d.n_atoms);                            // atoms_ws + blockIdx * n_atoms
    if (!d.boxes_in_lds) touch(boxes_ws, slots * 6 * n_boxes);     // boxes_ws + blockIdx * 6 * n_boxes
    touch(pairs_ws, slots * (size_t)d.n_rec_res * lw);             // pairs_ws + blockIdx * n_rec_res * lw
    peek(overflow, 1);                                             // set, never cleared, by the kernel
    if (offsets) peek(offsets, n + 1);
    std::vector<long long> xyz(3 * (size_t)d.n_atoms);
    for (size_t i = 0; i < n; i++) {
        for (int a = 0; a < d.n_atoms; a++) {
            int v[3];
            if (!posed_thousandths(m, poses + i * stride, (uint32_t)a, kComplexCoordBound, v)) *overflow = 1;
            for (int k = 0; k < 3; k++) xyz[3 * (size_t)a + k] = v[k];
        }
        uint32_t count = 0;
        size_t at = offsets ? offsets[i] : 0;
        for (int r = 0; r < d.n_rec_res; r++)
            for (int l = 0; l < d.n_lig_res; l++) {
                bool hit = false;
                for (uint32_t a = d.res_start[r]; a < d.res_start[r + 1] && !hit; a++)
                    for (uint32_t b = d.res_start[d.n_rec_res + l]; b < d.res_start[d.n_rec_res + l + 1] && !hit; b++) {
                        const long long dx = xyz[3 * a] - xyz[3 * b], dy = xyz[3 * a + 1] - xyz[3 * b + 1], dz = xyz[3 * a + 2] - xyz[3 * b + 2];
                        hit = std::llabs(dx) <= 30000 && std::llabs(dy) <= 30000 && std::llabs(dz) <= 30000 &&
                              dx * dx + dy * dy + dz * dz <= (long long)C2;
                    }
                if (!hit) continue;
                count++;
                if (offsets) keys[at++] = (uint32_t)r * (uint32_t)d.n_lig_res + (uint32_t)l;
            }
        if (!offsets) counts[i] = count;
        else if (at != offsets[i + 1]) return hipErrorInvalidValue;
    }
    return hipSuccess;
}

hipError_t launch_fcc_exclusive_scan(const uint32_t *in, size_t n, uint32_t *out, unsigned long long *total, hipStream_t) {
    unsigned long long running = 0;
    for (size_t i = 0; i < n; i++) {
        const uint32_t v = in[i];
        out[i] = (uint32_t)running;
        running += v;
    }
    out[n] = (uint32_t)running;
    *total = running;
    return hipSuccess;
}

hipError_t launch_fcc_mark(const uint32_t *keys, size_t total, uint32_t key_lo, uint32_t *bitmap, hipStream_t) {
    for (size_t x = 0; x < total; x++) {
        const uint32_t k = keys[x] - key_lo;
        bitmap[k >> 5] |= 1u << (k & 31);
    }
    return hipSuccess;
}

hipError_t launch_fcc_rank_counts(const uint32_t *bitmap, size_t n_rank, uint32_t *rank, hipStream_t) {
    for (size_t b = 0; b < n_rank; b++) {
        uint32_t count = 0;
        for (int w = 0; w < kFccRankWords; w++) count += (uint32_t)__builtin_popcount(bitmap[b * kFccRankWords + w]);
        rank[b] = count;
    }
    return hipSuccess;
}

hipError_t launch_fcc_rows(const uint32_t *offsets, const uint32_t *keys, size_t n, const uint32_t *row_of, uint32_t key_lo,
                           const uint32_t *bitmap, const uint32_t *rank, size_t W, uint32_t *rows, uint32_t *cols, uint32_t *freq,
                           uint32_t *sizes, hipStream_t) {
    touch(sizes, n);
    for (size_t i = 0; i < n; i++) {
        const size_t row = row_of ? row_of[i] : i;
        if (row >= n) return hipErrorInvalidValue;
        sizes[row] = offsets[i + 1] - offsets[i];
        for (size_t x = offsets[i]; x < offsets[i + 1]; x++) {
            const uint32_t k = keys[x] - key_lo;
            const size_t word = k >> 5;
            uint32_t col = rank[word / kFccRankWords];
            for (size_t w = word / kFccRankWords * kFccRankWords; w < word; w++) col += (uint32_t)__builtin_popcount(bitmap[w]);
            col += (uint32_t)__builtin_popcount(bitmap[word] & ((1u << (k & 31)) - 1u));
            if (!(bitmap[word] >> (k & 31) & 1u) || col >= 32 * W) return hipErrorInvalidValue;
            cols[x] = col;
            rows[row * W + (col >> 5)] |= 1u << (col & 31);
            freq[col]++;
        }
    }
    return hipSuccess;
}

// Row i's columns, ascending, from its bits.
static std::vector<uint32_t> columns(const uint32_t *rows, size_t W, size_t i) {
    std::vector<uint32_t> out;
    for (size_t w = 0; w < W; w++)
        for (int b = 0; b < 32; b++)
            if (rows[i * W + w] >> b & 1u) out.push_back((uint32_t)(32 * w + b));
    return out;
}

hipError_t launch_fcc_common(const uint32_t *rows, size_t W, size_t n, const uint32_t *sizes, uint32_t T, uint32_t *nbr, uint32_t *common,
                             hipStream_t) {
    if ((nbr == nullptr) == (common == nullptr) || n > kFccMaxSets || W == 0) return hipErrorInvalidValue;
    const size_t NW = (n + 31) / 32;
    peek(rows, n * W);
    peek(sizes, n);
    if (nbr) std::memset(nbr, 0, n * NW * sizeof(uint32_t));   // the kernel stores every word once
    else touch(common, n * n);
    std::vector<std::vector<uint32_t>> sets(n);
    for (size_t i = 0; i < n; i++) sets[i] = columns(rows, W, i);
    for (size_t i = 0; i < n; i++)
        for (size_t j = i; j < n; j++) {
            size_t a = 0, b = 0;
            uint32_t c = 0;
            while (a < sets[i].size() && b < sets[j].size()) {   // two sorted lists, merged
                if (sets[i][a] == sets[j][b]) c++, a++, b++;
                else if (sets[i][a] < sets[j][b]) a++;
                else b++;
            }
            if (common) common[i * n + j] = common[j * n + i] = c;
            else if (i != j && fcc_neighbours(c, sizes[i], sizes[j], T)) {
                nbr[i * NW + (j >> 5)] |= 1u << (j & 31);
                nbr[j * NW + (i >> 5)] |= 1u << (i & 31);
            }
        }
    return hipSuccess;
}

hipError_t launch_fcc_degrees(const uint32_t *nbr, size_t n, int *deg, hipStream_t) {
    const size_t NW = (n + 31) / 32;
    for (size_t i = 0; i < n; i++) {
        int count = 1;
        for (size_t w = 0; w < NW; w++) count += __builtin_popcount(nbr[i * NW + w]);
        deg[i] = count;
    }
    return hipSuccess;
}

// The rule's text, a round at a time, every count recounted: not the kernel's bookkeeping.
hipError_t launch_fcc_greedy(const uint32_t *nbr, size_t n, int *deg, uint32_t min_size, int *members, int32_t *cluster_of, int32_t *centres,
                             FccStatus *status, hipStream_t) {
    if (n > kFccMaxSets) return hipErrorInvalidValue;
    const size_t NW = (n + 31) / 32;
    peek(deg, n);
    touch(members, n);
    std::vector<char> alive(n, 1);
    for (size_t i = 0; i < n; i++) cluster_of[i] = centres[i] = -1;
    auto linked = [&](size_t i, size_t j) { return (nbr[i * NW + (j >> 5)] >> (j & 31) & 1u) != 0; };
    uint32_t cid = 0;
    for (;;) {
        long long best = -1, best_d = 0;
        for (size_t i = 0; i < n; i++) {
            if (!alive[i]) continue;
            long long d = 1;
            for (size_t j = 0; j < n; j++) d += alive[j] && linked(i, j);
            if (d > best_d) best_d = d, best = (long long)i;   // rows are in (scoring descending, index ascending) order
        }
        if (best < 0 || best_d < (long long)min_size) break;
        for (size_t j = 0; j < n; j++)
            if (alive[j] && (j == (size_t)best || linked((size_t)best, j))) cluster_of[j] = (int32_t)cid;
        for (size_t j = 0; j < n; j++)
            if (cluster_of[j] == (int32_t)cid) alive[j] = 0;
        centres[cid++] = (int32_t)best;
    }
    status->n_clusters = cid;
    status->rounds = cid;
    return hipSuccess;
}

hipError_t launch_fcc_consensus(const uint32_t *offsets, const uint32_t *cols, const uint32_t *freq, size_t n, unsigned long long *consensus,
                                hipStream_t) {
    for (size_t i = 0; i < n; i++) {
        unsigned long long sum = 0;
        for (size_t x = offsets[i]; x < offsets[i + 1]; x++) sum += freq[cols[x]];
        consensus[i] = sum;
    }
    return hipSuccess;
}

}  // namespace ld
