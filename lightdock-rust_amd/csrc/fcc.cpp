// fcc.cpp -- the host side of clustering by common contacts: argument checks, the workspace (blocks of several arrays laid
// out through device_memory.hpp's Carver) and the launch sequences of kernels/fcc.hpp, for a complex
// (Complex::pair_contacts, Complex::cluster_fcc) and for sets the caller gives.
#include "fcc.hpp"

#include <algorithm>
#include <cmath>
#include <string>

#include "complex.hpp"

namespace ld {

namespace {

thread_local double g_last_kernel_ms = 0.0;

// Offsets from 0 that ascend, keys strictly ascending inside a set -> the smallest key and the span of all keys.
void check_sets(size_t n, const uint32_t *offsets, const uint32_t *keys, uint32_t *key_lo, uint64_t *key_span) {
    if (!offsets) throw Error(LD_ERR_INVALID, "null offsets");
    if (offsets[0] != 0) throw Error(LD_ERR_INVALID, "offsets[0] must be 0");
    for (size_t i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i]) throw Error(LD_ERR_INVALID, "offsets do not ascend at set " + std::to_string(i));
    if (offsets[n] && !keys) throw Error(LD_ERR_INVALID, "null keys");
    uint32_t lo = 0xffffffffu, hi = 0;
    for (size_t i = 0; i < n; i++)
        for (size_t x = offsets[i]; x < offsets[i + 1]; x++) {
            if (x > offsets[i] && keys[x] <= keys[x - 1])
                throw Error(LD_ERR_INVALID, "the keys of set " + std::to_string(i) + " are not strictly ascending");
            lo = std::min(lo, keys[x]);
            hi = std::max(hi, keys[x]);
        }
    *key_lo = offsets[n] ? lo : 0;
    *key_span = offsets[n] ? (uint64_t)hi - lo + 1 : 1;
}

struct Uploaded {
    DeviceBuffer offsets, keys;
    FccCluster::Sets sets;
};

void upload_sets(size_t n, const uint32_t *offsets, const uint32_t *keys, Uploaded &u) {
    FccCluster::Sets &s = u.sets;
    check_sets(n, offsets, keys, &s.key_lo, &s.key_span);
    s.n = n;
    s.total = offsets[n];
    reserve_exact(u.offsets, (n + 1) * sizeof(uint32_t));
    reserve_exact(u.keys, std::max<size_t>(1, s.total) * sizeof(uint32_t));
    hip_check(hipMemcpy(u.offsets.ptr, offsets, (n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice), "hipMemcpy H2D offsets");
    if (s.total) hip_check(hipMemcpy(u.keys.ptr, keys, s.total * sizeof(uint32_t), hipMemcpyHostToDevice), "hipMemcpy H2D keys");
    s.d_offsets = static_cast<const uint32_t *>(u.offsets.ptr);
    s.d_keys = static_cast<const uint32_t *>(u.keys.ptr);
}

// HIP events around a call on the null stream.
struct Timed {
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    Timed() {
        hip_check(hipEventCreate(&ev0), "hipEventCreate");
        if (hipEventCreate(&ev1) != hipSuccess) {
            (void)hipEventDestroy(ev0);
            throw Error(LD_ERR_DEVICE, "hipEventCreate");
        }
        hip_check(hipEventRecord(ev0, nullptr), "hipEventRecord");
    }
    ~Timed() {
        (void)hipEventDestroy(ev0);
        (void)hipEventDestroy(ev1);
    }
    void stop() {
        hip_check(hipEventRecord(ev1, nullptr), "hipEventRecord");
        hip_check(hipEventSynchronize(ev1), "hipEventSynchronize");
        float ms = 0.0f;
        hip_check(hipEventElapsedTime(&ms, ev0, ev1), "hipEventElapsedTime");
        g_last_kernel_ms = ms;
    }
};

}  // namespace

double fcc_last_kernel_ms() { return g_last_kernel_ms; }

uint32_t fcc_threshold(double threshold) {
    const char *message = "threshold must be 0.001 .. 1";
    const double scaled = threshold * 1000.0;
    if (!(scaled > 0.0 && scaled < 1001.0)) throw Error(LD_ERR_INVALID, message);
    const long long T = std::llrint(scaled);
    if (T < 1 || T > 1000) throw Error(LD_ERR_INVALID, message);
    return (uint32_t)T;
}

// The union of all keys renumbered densely (a presence bitmap over the span of the keys, ranks every 1024 keys), then every
// set as a bit row of W words.  Leaves sizes_ (by row), cols_ (a column a key) and freq_ (sets a column).
size_t FccCluster::build_rows(const Sets &s, const uint32_t *d_row_of, hipStream_t stream) {
    const size_t n_rank = (size_t)((s.key_span + 32 * kFccRankWords - 1) / (32 * kFccRankWords));
    reserve_exact(status_, sizeof(FccStatus));
    reserve_exact(bitmap_, n_rank * kFccRankWords * sizeof(uint32_t));
    reserve_exact(rank_, (n_rank + 1) * sizeof(uint32_t));
    FccStatus *d_status = static_cast<FccStatus *>(status_.ptr);
    uint32_t *d_bitmap = static_cast<uint32_t *>(bitmap_.ptr), *d_rank = static_cast<uint32_t *>(rank_.ptr);
    hip_check(hipMemsetAsync(d_bitmap, 0, n_rank * kFccRankWords * sizeof(uint32_t), stream), "hipMemset");
    if (s.total) hip_check(launch_fcc_mark(s.d_keys, s.total, s.key_lo, d_bitmap, stream), "fcc_mark launch");
    hip_check(launch_fcc_rank_counts(d_bitmap, n_rank, d_rank, stream), "fcc_rank_counts launch");
    hip_check(launch_fcc_exclusive_scan(d_rank, n_rank, d_rank, &d_status->total, stream), "fcc_exclusive_scan launch");
    FccStatus st;
    hip_check(hipMemcpyAsync(&st, d_status, sizeof st, hipMemcpyDeviceToHost, stream), "hipMemcpy D2H status");
    hip_check(hipStreamSynchronize(stream), "fcc renumbering");
    const size_t U = (size_t)st.total, W = std::max<size_t>(1, (U + 31) / 32);
    if (s.n * W * sizeof(uint32_t) > kFccMaxRowBytes)
        throw Error(LD_ERR_INVALID, "the bit rows of " + std::to_string(s.n) + " sets over " + std::to_string(U) + " distinct keys would exceed 1 GiB");
    reserve_exact(rows_, s.n * W * sizeof(uint32_t));
    reserve_exact(cols_, std::max<size_t>(1, s.total) * sizeof(uint32_t));
    reserve_exact(freq_, std::max<size_t>(1, U) * sizeof(uint32_t));
    reserve_exact(sizes_, s.n * sizeof(uint32_t));
    hip_check(hipMemsetAsync(rows_.ptr, 0, s.n * W * sizeof(uint32_t), stream), "hipMemset");
    hip_check(hipMemsetAsync(freq_.ptr, 0, std::max<size_t>(1, U) * sizeof(uint32_t), stream), "hipMemset");
    hip_check(launch_fcc_rows(s.d_offsets, s.d_keys, s.n, d_row_of, s.key_lo, d_bitmap, d_rank, W, static_cast<uint32_t *>(rows_.ptr),
                              static_cast<uint32_t *>(cols_.ptr), static_cast<uint32_t *>(freq_.ptr), static_cast<uint32_t *>(sizes_.ptr),
                              stream),
              "fcc_rows launch");
    return W;
}

void FccCluster::cluster(const Sets &s, const double *scoring, uint32_t T, uint32_t min_size, bool consensus, hipStream_t stream,
                         Result &out) {
    const size_t n = s.n;
    // (scoring descending, index ascending): a set's row is its place in that order, so the kernels break ties by row
    std::vector<uint32_t> order(n), row_of(n);
    for (size_t i = 0; i < n; i++) order[i] = (uint32_t)i;
    std::stable_sort(order.begin(), order.end(), [scoring](uint32_t a, uint32_t b) { return scoring[a] > scoring[b]; });
    for (size_t p = 0; p < n; p++) row_of[order[p]] = (uint32_t)p;

    uint32_t *d_row_of;
    int *d_deg, *d_members;
    int32_t *d_cluster, *d_centres;
    carve_into(work_, [&](Carver &c) {
        d_row_of = c.take<uint32_t>(n), d_deg = c.take<int>(n), d_members = c.take<int>(n);
        d_cluster = c.take<int32_t>(n), d_centres = c.take<int32_t>(n);
    });
    hip_check(hipMemcpyAsync(d_row_of, row_of.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, stream), "hipMemcpy H2D rows");
    const size_t W = build_rows(s, d_row_of, stream);

    const size_t NW = (n + 31) / 32;
    reserve_exact(nbr_, n * NW * sizeof(uint32_t));
    uint32_t *d_nbr = static_cast<uint32_t *>(nbr_.ptr);
    FccStatus *d_status = static_cast<FccStatus *>(status_.ptr);
    hip_check(launch_fcc_common(static_cast<const uint32_t *>(rows_.ptr), W, n, static_cast<const uint32_t *>(sizes_.ptr), T, d_nbr, nullptr,
                                stream),
              "fcc_common launch");
    hip_check(launch_fcc_degrees(d_nbr, n, d_deg, stream), "fcc_degrees launch");
    hip_check(launch_fcc_greedy(d_nbr, n, d_deg, min_size, d_members, d_cluster, d_centres, d_status, stream), "fcc_greedy launch");
    std::vector<int32_t> by_row(n), centre_rows(n);
    out.consensus.assign(consensus ? n : 0, 0);
    if (consensus) {
        reserve_exact(out_, n * sizeof(unsigned long long));
        hip_check(launch_fcc_consensus(s.d_offsets, static_cast<const uint32_t *>(cols_.ptr), static_cast<const uint32_t *>(freq_.ptr), n,
                                       static_cast<unsigned long long *>(out_.ptr), stream),
                  "fcc_consensus launch");
        hip_check(hipMemcpyAsync(out.consensus.data(), out_.ptr, n * sizeof(uint64_t), hipMemcpyDeviceToHost, stream), "hipMemcpy D2H");
    }
    FccStatus st;
    hip_check(hipMemcpyAsync(&st, d_status, sizeof st, hipMemcpyDeviceToHost, stream), "hipMemcpy D2H status");
    hip_check(hipMemcpyAsync(by_row.data(), d_cluster, n * sizeof(int32_t), hipMemcpyDeviceToHost, stream), "hipMemcpy D2H");
    hip_check(hipMemcpyAsync(centre_rows.data(), d_centres, n * sizeof(int32_t), hipMemcpyDeviceToHost, stream), "hipMemcpy D2H");
    hip_check(hipStreamSynchronize(stream), "fcc clustering");
    if (st.n_clusters > n) throw Error(LD_ERR_DEVICE, "fcc clustering: more clusters than sets");
    out.n_clusters = st.n_clusters;
    out.rounds = st.rounds;
    out.cluster_of.resize(n);
    out.centres.resize(n);
    for (size_t p = 0; p < n; p++) out.cluster_of[order[p]] = by_row[p];
    for (size_t c = 0; c < n; c++) out.centres[c] = c < st.n_clusters ? (int32_t)order[(size_t)centre_rows[c]] : -1;
}

void FccCluster::common(const Sets &s, uint32_t *common_out, hipStream_t stream) {
    const size_t n = s.n, W = build_rows(s, nullptr, stream);
    reserve_exact(out_, n * n * sizeof(uint32_t));
    hip_check(launch_fcc_common(static_cast<const uint32_t *>(rows_.ptr), W, n, static_cast<const uint32_t *>(sizes_.ptr), 1, nullptr,
                                static_cast<uint32_t *>(out_.ptr), stream),
              "fcc_common launch");
    hip_check(hipMemcpyAsync(common_out, out_.ptr, n * n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream), "hipMemcpy D2H");
    hip_check(hipStreamSynchronize(stream), "fcc_common");
}

void fcc_common_host(size_t n, const uint32_t *offsets, const uint32_t *keys, uint32_t *common) {
    if (n > kFccMaxCommonSets) throw Error(LD_ERR_INVALID, "more than 16384 sets: the n x n words would exceed 1 GiB");
    g_last_kernel_ms = 0.0;
    if (n == 0) return;
    if (!common) throw Error(LD_ERR_INVALID, "null argument");
    Uploaded u;
    upload_sets(n, offsets, keys, u);
    std::vector<uint32_t> result(n * n);
    FccCluster f;
    Timed timed;
    f.common(u.sets, result.data(), nullptr);
    timed.stop();
    std::copy(result.begin(), result.end(), common);
}

void fcc_cluster_host(size_t n, const uint32_t *offsets, const uint32_t *keys, const double *scoring, double threshold,
                      uint32_t min_size, int32_t *cluster_of, int32_t *centres, uint32_t *n_clusters, uint64_t *consensus) {
    const uint32_t T = fcc_threshold(threshold);
    if (min_size == 0) throw Error(LD_ERR_INVALID, "min_size must be 1 at least");
    if (!n_clusters) throw Error(LD_ERR_INVALID, "null argument");
    if (n > kFccMaxSets) throw Error(LD_ERR_INVALID, "more than 65536 sets: the neighbour bits would exceed 512 MiB");
    g_last_kernel_ms = 0.0;
    if (n == 0) {
        *n_clusters = 0;
        return;
    }
    if (!scoring || !cluster_of || !centres) throw Error(LD_ERR_INVALID, "null argument");
    check_scoring(n, scoring);
    Uploaded u;
    upload_sets(n, offsets, keys, u);
    FccCluster f;
    FccCluster::Result r;
    Timed timed;
    f.cluster(u.sets, scoring, T, min_size, consensus != nullptr, nullptr, r);
    timed.stop();
    std::copy(r.cluster_of.begin(), r.cluster_of.end(), cluster_of);
    std::copy(r.centres.begin(), r.centres.end(), centres);
    *n_clusters = r.n_clusters;
    if (consensus) std::copy(r.consensus.begin(), r.consensus.end(), consensus);
}

// --- a complex's pair sets ---------------------------------------------------------------------------------------------

// Count pass, scan and, with `fill`, the keys: the sets of n checked poses as CSR on the device (offsets in d_ids_, keys in
// d_pair_keys_).  begin_timed stands in front of the first launch; the caller ends the timing with finish_timed(*d_overflow).
FccCluster::Sets Complex::pair_sets(size_t n, const double *poses, size_t stride, long long C, bool fill, size_t cap, int **d_overflow_out) {
    const ContactsDevice &k = contacts_;
    const size_t lw = ((size_t)k.n_lig_res + 31) / 32, pair_words = (size_t)k.n_rec_res * lw;
    const size_t per_slot = (size_t)k.n_atoms * sizeof(int4) + (k.boxes_in_lds ? 0 : k.box_bytes()) + pair_words * sizeof(uint32_t);
    const size_t slots = chunk_of(per_slot, n, kPairSlots);
    upload_poses(n, poses, stride);
    FccStatus *d_status;
    int *d_overflow, *d_boxes;
    uint32_t *d_counts, *d_offsets, *d_pairs;
    int4 *d_atoms;
    carve_into(d_ids_, [&](Carver &c) {
        d_status = c.take<FccStatus>(1), d_overflow = c.take<int>(1), d_counts = c.take<uint32_t>(n), d_offsets = c.take<uint32_t>(n + 1);
    });
    carve_into(d_ws_, [&](Carver &c) {
        d_atoms = c.take<int4>(slots * k.n_atoms), d_boxes = c.take<int>(k.boxes_in_lds ? 0 : slots * 6 * (size_t)k.n_boxes());
        d_pairs = c.take<uint32_t>(slots * pair_words);
    });
    const double *d_poses = static_cast<const double *>(d_poses_.ptr);
    const char *beyond = "a posed coordinate is beyond +-1.0e6 A";
    begin_timed(d_overflow);
    hip_check(launch_complex_pair_sets(dev_, k, d_poses, stride, n, (uint32_t)(C * C), slots, d_atoms, d_boxes, d_pairs, nullptr, d_counts,
                                       nullptr, d_overflow, stream_),
              "complex_pair_sets launch");
    hip_check(launch_fcc_exclusive_scan(d_counts, n, d_offsets, &d_status->total, stream_), "fcc_exclusive_scan launch");
    FccStatus st;
    int overflow = 0;
    hip_check(hipMemcpyAsync(&st, d_status, sizeof st, hipMemcpyDeviceToHost, stream_), "hipMemcpy D2H status");
    hip_check(hipMemcpyAsync(&overflow, d_overflow, sizeof(int), hipMemcpyDeviceToHost, stream_), "hipMemcpy D2H");
    hip_check(hipStreamSynchronize(stream_), "complex_pair_sets");
    if (overflow) throw Error(LD_ERR_INVALID, beyond);
    if (st.total > 0xffffffffull) throw Error(LD_ERR_INVALID, "more than 2^32 - 1 residue pairs in contact over the list");
    FccCluster::Sets s;
    s.n = n;
    s.total = (size_t)st.total;
    s.d_offsets = d_offsets;
    s.key_lo = 0;
    s.key_span = std::max<uint64_t>(1, (uint64_t)k.n_rec_res * (uint64_t)k.n_lig_res);
    if (fill) {
        if (cap < s.total)
            throw Error(LD_ERR_INVALID, "room for " + std::to_string(cap) + " keys, the list has " + std::to_string(s.total));
        reserve_exact(d_pair_keys_, std::max<size_t>(1, s.total) * sizeof(uint32_t));
        uint32_t *d_keys = static_cast<uint32_t *>(d_pair_keys_.ptr);
        hip_check(launch_complex_pair_sets(dev_, k, d_poses, stride, n, (uint32_t)(C * C), slots, d_atoms, d_boxes, d_pairs, d_offsets,
                                           d_counts, d_keys, d_overflow, stream_),
                  "complex_pair_sets launch");
        s.d_keys = d_keys;
    }
    *d_overflow_out = d_overflow;
    return s;
}

void Complex::check_pair_keys() const {
    if ((uint64_t)contacts_.n_rec_res * (uint64_t)contacts_.n_lig_res >= (uint64_t(1) << 32))
        throw Error(LD_ERR_INVALID, "receptor residues x ligand residues must be below 2^32: a pair is a 32-bit key");
}

void Complex::pair_contacts(size_t n, const double *poses, size_t stride, double cutoff, uint32_t *offsets, uint32_t *keys, size_t cap,
                            size_t *total_out) {
    const long long C = cutoff_thousandths(cutoff, "cutoff must be 0.001 .. 30 A");
    check_pair_keys();
    if (n > kFccMaxPoses) throw Error(LD_ERR_INVALID, "more than 4194304 poses in one call");
    if (n == 0) {
        if (offsets) offsets[0] = 0;
        if (total_out) *total_out = 0;
        return;
    }
    check_poses(n, poses, stride);
    int *d_overflow = nullptr;
    const FccCluster::Sets s = pair_sets(n, poses, stride, C, keys != nullptr, cap, &d_overflow);
    finish_timed(d_overflow, "complex_pair_sets", "a posed coordinate is beyond +-1.0e6 A");
    if (offsets) hip_check(hipMemcpy(offsets, s.d_offsets, (n + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost), "hipMemcpy D2H");
    if (keys && s.total) hip_check(hipMemcpy(keys, s.d_keys, s.total * sizeof(uint32_t), hipMemcpyDeviceToHost), "hipMemcpy D2H");
    if (total_out) *total_out = s.total;
}

void Complex::cluster_fcc(size_t n, const double *poses, size_t stride, const double *scoring, double cutoff, double threshold,
                          uint32_t min_size, int32_t *cluster_of, int32_t *centres, uint32_t *n_clusters, uint32_t *set_sizes,
                          uint64_t *consensus) {
    const long long C = cutoff_thousandths(cutoff, "cutoff must be 0.001 .. 30 A");
    const uint32_t T = fcc_threshold(threshold);
    if (min_size == 0) throw Error(LD_ERR_INVALID, "min_size must be 1 at least");
    check_pair_keys();
    if (!n_clusters) throw Error(LD_ERR_INVALID, "null argument");
    // the bound comes before anything reads the list
    if (n > kFccMaxSets) throw Error(LD_ERR_INVALID, "more than 65536 poses: the neighbour bits would exceed 512 MiB");
    if (n == 0) {
        *n_clusters = 0;
        return;
    }
    if (!scoring || !cluster_of || !centres) throw Error(LD_ERR_INVALID, "null argument");
    check_poses(n, poses, stride);
    check_scoring(n, scoring);
    int *d_overflow = nullptr;
    const FccCluster::Sets s = pair_sets(n, poses, stride, C, true, SIZE_MAX, &d_overflow);
    FccCluster::Result r;
    fcc_.cluster(s, scoring, T, min_size, consensus != nullptr, stream_, r);
    finish_timed(d_overflow, "complex_cluster_fcc", "a posed coordinate is beyond +-1.0e6 A");
    if (set_sizes) {
        std::vector<uint32_t> offsets(n + 1);
        hip_check(hipMemcpy(offsets.data(), s.d_offsets, (n + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost), "hipMemcpy D2H");
        for (size_t i = 0; i < n; i++) set_sizes[i] = offsets[i + 1] - offsets[i];
    }
    std::copy(r.cluster_of.begin(), r.cluster_of.end(), cluster_of);
    std::copy(r.centres.begin(), r.centres.end(), centres);
    *n_clusters = r.n_clusters;
    if (consensus) std::copy(r.consensus.begin(), r.consensus.end(), consensus);
}

}  // namespace ld
