// fcc_check.cpp -- driver of the sanitizer build of clustering by common contacts (`make asan-fcc`; tests/test_asan_fcc.py):
// ld_fcc_common / ld_fcc_cluster / ld_complex_pair_contacts / ld_complex_cluster_fcc through the C ABI against
// tests/asan/hip_stub.cpp and tests/asan/hip_stub_fcc.cpp (device memory = host memory; the launches do the kernels' work
// in plain C++ from the shared rule, so the answers are real ones): hand-made sets whose clusters the rule's text pins, three
// 1czy poses, every NULL / non-NULL combination of the outputs, and every refusal by status with the outputs untouched.
//   usage: fcc_check <tests/golden> <scratch dir>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#define CHECK_PROGRAM "fcc_check"
#include "check.hpp"
#include "host/io.hpp"

static const uint32_t M32 = 0xA5A5A5A5u;
static const uint64_t M64 = 0xA5A5A5A5A5A5A5A5ull;

struct Out {
    std::vector<int32_t> cluster_of, centres;
    uint32_t n_clusters = M32;
    std::vector<uint32_t> sizes;
    std::vector<uint64_t> consensus;
    explicit Out(size_t n) : cluster_of(n, -7), centres(n, -7), sizes(n, M32), consensus(n, M64) {}
    bool untouched() const {
        for (size_t i = 0; i < cluster_of.size(); i++)
            if (cluster_of[i] != -7 || centres[i] != -7 || sizes[i] != M32 || consensus[i] != M64) return false;
        return n_clusters == M32;
    }
};

struct Sets {
    std::vector<uint32_t> offsets{0}, keys;
    void add(std::initializer_list<uint32_t> s) {
        keys.insert(keys.end(), s);
        offsets.push_back((uint32_t)keys.size());
    }
    size_t n() const { return offsets.size() - 1; }
};

static int cluster(const Sets &s, const std::vector<double> &scoring, double threshold, uint32_t min_size, Out &o, bool consensus = true) {
    return ld_fcc_cluster(s.n(), s.offsets.data(), s.keys.data(), scoring.data(), threshold, min_size, o.cluster_of.data(), o.centres.data(),
                          &o.n_clusters, consensus ? o.consensus.data() : nullptr);
}

static void hand_made() {
    // 0, 1, 2 share {1, 2, 3} of four keys each (3/4 >= 0.6); 3 is empty; 4 and 5 are one set twice; 6 is alone
    Sets s;
    s.add({1, 2, 3, 4});
    s.add({1, 2, 3, 5});
    s.add({1, 2, 3, 6});
    s.add({});
    s.add({4000000000u, 4000000001u});
    s.add({4000000000u, 4000000001u});
    s.add({77});
    const std::vector<double> flat(7, 0.0);
    Out o(7);
    CHECK(cluster(s, flat, 0.6, 1, o) == LD_OK && o.n_clusters == 4);
    CHECK((o.cluster_of == std::vector<int32_t>{0, 0, 0, 2, 1, 1, 3}));          // singletons by index: 3 before 6
    CHECK((o.centres == std::vector<int32_t>{0, 4, 3, 6, -1, -1, -1}));          // ties in d and scoring: the smaller index
    CHECK((o.consensus == std::vector<uint64_t>{10, 10, 10, 0, 4, 4, 1}));
    // the larger scoring wins a tie in d, before the index
    std::vector<double> scored = {0.0, 2.0, 1.0, 9.0, -1.0, 5.0, 0.5};
    Out p(7);
    CHECK(cluster(s, scored, 0.6, 1, p) == LD_OK && p.n_clusters == 4);
    CHECK((p.centres == std::vector<int32_t>{1, 5, 3, 6, -1, -1, -1}) && (p.cluster_of == std::vector<int32_t>{0, 0, 0, 2, 1, 1, 3}));
    // min_size 2 leaves the singletons at -1; min_size 8 everything
    Out q(7);
    CHECK(cluster(s, scored, 0.6, 2, q) == LD_OK && q.n_clusters == 2);
    CHECK((q.cluster_of == std::vector<int32_t>{0, 0, 0, -1, 1, 1, -1}) && (q.centres == std::vector<int32_t>{1, 5, -1, -1, -1, -1, -1}));
    Out r(7);
    CHECK(cluster(s, scored, 0.6, 8, r) == LD_OK && r.n_clusters == 0);
    CHECK((r.cluster_of == std::vector<int32_t>(7, -1)) && (r.centres == std::vector<int32_t>(7, -1)));
    // at 0.76 nothing but the identical sets is left
    Out t(7);
    CHECK(cluster(s, flat, 0.76, 1, t) == LD_OK && t.n_clusters == 6 && t.cluster_of[4] == 0 && t.cluster_of[5] == 0 && t.cluster_of[0] == 1);
    // exactly on the threshold, and one key short of it
    Sets on, shy;
    on.add({1, 2, 3, 4, 5});
    on.add({3, 4, 5, 8, 9});
    shy.add({1, 2, 3, 4, 5});
    shy.add({3, 4, 5, 8, 9, 10});
    Out a(2), b(2);
    CHECK(cluster(on, {0.0, 1.0}, 0.6, 1, a) == LD_OK && a.n_clusters == 1 && a.centres[0] == 1 && a.cluster_of[0] == 0);
    CHECK(cluster(shy, {0.0, 1.0}, 0.6, 1, b) == LD_OK && b.n_clusters == 2 && b.cluster_of[0] == 1 && b.cluster_of[1] == 0);
    // common contacts
    std::vector<uint32_t> c(49, M32);
    CHECK(ld_fcc_common(7, s.offsets.data(), s.keys.data(), c.data()) == LD_OK);
    CHECK(c[0] == 4 && c[1] == 3 && c[7] == 3 && c[2 * 7 + 1] == 3 && c[3 * 7 + 3] == 0 && c[4 * 7 + 5] == 2 && c[6 * 7 + 6] == 1 && c[6] == 0);
    double ms = -1.0;
    CHECK(ld_fcc_last_kernel_ms(&ms) == LD_OK && ms == 0.0 && ld_fcc_last_kernel_ms(nullptr) == LD_ERR_INVALID);
    // consensus is optional
    Out u(7);
    CHECK(cluster(s, flat, 0.6, 1, u, false) == LD_OK && u.cluster_of == o.cluster_of && u.consensus == std::vector<uint64_t>(7, M64));
    uint32_t k = M32;
    CHECK(ld_fcc_cluster(0, nullptr, nullptr, nullptr, 0.6, 1, nullptr, nullptr, &k, nullptr) == LD_OK && k == 0);
    CHECK(ld_fcc_common(0, nullptr, nullptr, nullptr) == LD_OK);

    // refusals: nothing written
    auto refused = [&](const Sets &bad, const std::vector<double> &sc, double threshold, uint32_t min_size, size_t n) {
        Out w(7);
        const int rc = ld_fcc_cluster(n, bad.offsets.data(), bad.keys.data(), sc.data(), threshold, min_size, w.cluster_of.data(), w.centres.data(),
                                      &w.n_clusters, w.consensus.data());
        return rc == LD_ERR_INVALID && w.untouched();
    };
    for (double threshold : {(double)NAN, 0.0, 0.0004, 1.0006, -1.0, 1e300, (double)INFINITY}) CHECK(refused(s, flat, threshold, 1, 7));
    CHECK(refused(s, flat, 0.6, 0, 7));
    CHECK(refused(s, flat, 0.6, 1, (size_t)1 << 40) && refused(s, flat, 0.6, 1, 65537));
    std::vector<double> nan_score = flat;
    nan_score[6] = NAN;
    CHECK(refused(s, nan_score, 0.6, 1, 7));
    nan_score[6] = -INFINITY;
    CHECK(refused(s, nan_score, 0.6, 1, 7));
    Sets down = s, from1 = s, twice = s, back = s;
    down.offsets[2] = 3;
    from1.offsets[0] = 1;
    twice.keys[1] = 1;
    back.keys[2] = 1;
    for (const Sets *bad : {&down, &from1, &twice, &back}) {
        CHECK(refused(*bad, flat, 0.6, 1, 7));
        std::vector<uint32_t> cc(49, M32);
        CHECK(ld_fcc_common(7, bad->offsets.data(), bad->keys.data(), cc.data()) == LD_ERR_INVALID && cc == std::vector<uint32_t>(49, M32));
    }
    std::vector<uint32_t> cc(49, M32);
    CHECK(ld_fcc_common(16385, s.offsets.data(), s.keys.data(), cc.data()) == LD_ERR_INVALID && cc == std::vector<uint32_t>(49, M32));
    CHECK(ld_fcc_common(7, nullptr, s.keys.data(), cc.data()) == LD_ERR_INVALID && ld_fcc_common(7, s.offsets.data(), nullptr, cc.data()) == LD_ERR_INVALID);
    CHECK(ld_fcc_common(7, s.offsets.data(), s.keys.data(), nullptr) == LD_ERR_INVALID);
    Out w(7);
    CHECK(ld_fcc_cluster(7, s.offsets.data(), s.keys.data(), nullptr, 0.6, 1, w.cluster_of.data(), w.centres.data(), &w.n_clusters, nullptr) == LD_ERR_INVALID);
    CHECK(ld_fcc_cluster(7, s.offsets.data(), s.keys.data(), flat.data(), 0.6, 1, nullptr, w.centres.data(), &w.n_clusters, nullptr) == LD_ERR_INVALID);
    CHECK(ld_fcc_cluster(7, s.offsets.data(), s.keys.data(), flat.data(), 0.6, 1, w.cluster_of.data(), nullptr, &w.n_clusters, nullptr) == LD_ERR_INVALID);
    CHECK(ld_fcc_cluster(7, s.offsets.data(), s.keys.data(), flat.data(), 0.6, 1, w.cluster_of.data(), w.centres.data(), nullptr, nullptr) == LD_ERR_INVALID);
    CHECK(w.untouched());
}

// Row `glowworm` of a gso_<step>.out: the numbers between its parentheses.
static std::vector<double> gso_pose(const std::string &path, int glowworm) {
    std::ifstream in(path);
    std::string line;
    int row = 0;
    while (std::getline(in, line)) {
        if (line.empty() || line[0] != '(') continue;
        if (row++ != glowworm) continue;
        std::vector<double> pose;
        const char *p = line.c_str() + 1;
        for (;;) {
            char *end = nullptr;
            pose.push_back(std::strtod(p, &end));
            if (*end != ',') break;
            p = end + 1;
        }
        return pose;
    }
    return {};
}

static void czy(const std::string &golden) {
    const std::string d = golden + "/1czy/";
    const std::vector<double> rec_nm = ld::read_npy_f64(d + "lightdock_rec.nm.npy"), lig_nm = ld::read_npy_f64(d + "lightdock_lig.nm.npy");
    ld_complex *c = ld_complex_create((d + "lightdock_1czy_protein.pdb").c_str(), (d + "lightdock_1czy_peptide.pdb").c_str(), rec_nm.data(),
                                      rec_nm.size(), 10, lig_nm.data(), lig_nm.size(), 10);
    CHECK(c != nullptr);
    if (!c) return;
    const size_t len = ld_complex_pose_len(c), stride = len + 2, n = 3;
    const size_t n_rec_res = ld_complex_num_residues(c, 0), n_lig_res = ld_complex_num_residues(c, 1);
    CHECK(len == 27 && n_rec_res == 168 && n_lig_res == 7);
    std::vector<double> poses(n * stride, 0.0);
    const std::vector<double> first = gso_pose(d + "swarm_2/gso_100.out", 74), second = gso_pose(d + "swarm_0/gso_100.out", 0),
                              third = gso_pose(d + "swarm_2/gso_100.out", 75);
    CHECK(first.size() == 27 && second.size() == 27 && third.size() == 27);
    if (first.size() != 27 || second.size() != 27 || third.size() != 27) return;
    std::copy(first.begin(), first.end(), poses.begin());
    std::copy(second.begin(), second.end(), poses.begin() + stride);
    std::copy(third.begin(), third.end(), poses.begin() + 2 * stride);
    const std::vector<double> scoring = {3.0, 2.0, 1.0};

    // the count protocol, then the keys
    std::vector<uint32_t> offsets(n + 1, M32);
    size_t total = 7;
    CHECK(ld_complex_pair_contacts(c, n, poses.data(), stride, 5.0, offsets.data(), nullptr, 0, &total) == LD_OK);
    CHECK(offsets[0] == 0 && offsets[3] == total && total > 0 && total < 3 * 168 * 7);
    std::vector<uint32_t> keys(total + 2, M32), again(n + 1, M32);
    CHECK(ld_complex_pair_contacts(c, n, poses.data(), stride, 5.0, again.data(), keys.data(), total, nullptr) == LD_OK && again == offsets);
    CHECK(keys[total] == M32 && keys[total + 1] == M32);
    bool ascending = true;
    for (size_t i = 0; i < n; i++)
        for (size_t x = offsets[i]; x < offsets[i + 1]; x++) ascending = ascending && keys[x] < n_rec_res * n_lig_res && (x == offsets[i] || keys[x] > keys[x - 1]);
    CHECK(ascending);
    // the residues the pairs name (the stub of ld_complex_contacts computes nothing to compare them with)
    std::vector<uint32_t> rec_want(n * 6, 0), lig_want(n, 0);
    for (size_t i = 0; i < n; i++)
        for (size_t x = offsets[i]; x < offsets[i + 1]; x++) {
            const uint32_t r = keys[x] / (uint32_t)n_lig_res, l = keys[x] % (uint32_t)n_lig_res;
            rec_want[i * 6 + (r >> 5)] |= 1u << (r & 31);
            lig_want[i] |= 1u << l;
        }
    CHECK(lig_want[0] != 0 && rec_want != std::vector<uint32_t>(n * 6, 0));
    // a cap too small: nothing written
    std::vector<uint32_t> small(total, M32);
    std::fill(again.begin(), again.end(), M32);
    size_t t2 = 7;
    CHECK(ld_complex_pair_contacts(c, n, poses.data(), stride, 5.0, again.data(), small.data(), total - 1, &t2) == LD_ERR_INVALID);
    CHECK(t2 == 7 && again == std::vector<uint32_t>(n + 1, M32) && small == std::vector<uint32_t>(total, M32));
    CHECK(ld_complex_pair_contacts(c, n, poses.data(), stride, 5.0, nullptr, nullptr, 0, nullptr) == LD_OK);
    CHECK(ld_complex_pair_contacts(c, 0, nullptr, stride, 5.0, again.data(), nullptr, 0, &t2) == LD_OK && again[0] == 0 && again[1] == M32 && t2 == 0);

    // the two steps in one call equal the two calls
    keys.resize(total);
    Out two(n), one(n);
    CHECK(ld_fcc_cluster(n, offsets.data(), keys.data(), scoring.data(), 0.5, 1, two.cluster_of.data(), two.centres.data(), &two.n_clusters,
                         two.consensus.data()) == LD_OK);
    CHECK(ld_complex_cluster_fcc(c, n, poses.data(), stride, scoring.data(), 5.0, 0.5, 1, one.cluster_of.data(), one.centres.data(),
                                 &one.n_clusters, one.sizes.data(), one.consensus.data()) == LD_OK);
    CHECK(one.cluster_of == two.cluster_of && one.centres == two.centres && one.n_clusters == two.n_clusters && one.consensus == two.consensus);
    CHECK(one.n_clusters >= 1 && one.n_clusters <= 3 && one.cluster_of[0] == 0);
    for (size_t i = 0; i < n; i++) CHECK(one.sizes[i] == offsets[i + 1] - offsets[i] && one.consensus[i] >= one.sizes[i]);
    // every NULL / non-NULL combination of the optional outputs
    for (int mask = 0; mask < 4; mask++) {
        Out p(n);
        CHECK(ld_complex_cluster_fcc(c, n, poses.data(), stride, scoring.data(), 5.0, 0.5, 1, p.cluster_of.data(), p.centres.data(), &p.n_clusters,
                                     mask & 1 ? p.sizes.data() : nullptr, mask & 2 ? p.consensus.data() : nullptr) == LD_OK);
        CHECK(p.cluster_of == one.cluster_of && p.centres == one.centres && p.n_clusters == one.n_clusters);
        CHECK(p.sizes == (mask & 1 ? one.sizes : std::vector<uint32_t>(n, M32)) && p.consensus == (mask & 2 ? one.consensus : std::vector<uint64_t>(n, M64)));
    }
    uint32_t k = M32;
    CHECK(ld_complex_cluster_fcc(c, 0, nullptr, stride, nullptr, 5.0, 0.5, 1, nullptr, nullptr, &k, nullptr, nullptr) == LD_OK && k == 0);

    // refusals: nothing written
    auto refused = [&](ld_complex *h, size_t count, const double *p, size_t st, const double *sc, double cutoff, double threshold, uint32_t min_size) {
        Out w(n);
        const int rc = ld_complex_cluster_fcc(h, count, p, st, sc, cutoff, threshold, min_size, w.cluster_of.data(), w.centres.data(), &w.n_clusters,
                                              w.sizes.data(), w.consensus.data());
        return rc == LD_ERR_INVALID && w.untouched();
    };
    auto pairs_refused = [&](ld_complex *h, size_t count, const double *p, size_t st, double cutoff) {
        std::vector<uint32_t> o(n + 1, M32), kk(total, M32);
        size_t t = 7;
        return ld_complex_pair_contacts(h, count, p, st, cutoff, o.data(), kk.data(), total, &t) == LD_ERR_INVALID && t == 7 &&
               o == std::vector<uint32_t>(n + 1, M32) && kk == std::vector<uint32_t>(total, M32);
    };
    for (double cutoff : {30.001, 0.0, -1.0, (double)NAN, 1e300}) {
        CHECK(refused(c, n, poses.data(), stride, scoring.data(), cutoff, 0.5, 1));
        CHECK(pairs_refused(c, n, poses.data(), stride, cutoff));
    }
    for (double threshold : {(double)NAN, 0.0, 1.0006, -0.5, (double)INFINITY}) CHECK(refused(c, n, poses.data(), stride, scoring.data(), 5.0, threshold, 1));
    CHECK(refused(c, n, poses.data(), stride, scoring.data(), 5.0, 0.5, 0));
    std::vector<double> bad = poses;
    bad[stride + 5] = NAN;
    CHECK(refused(c, n, bad.data(), stride, scoring.data(), 5.0, 0.5, 1) && pairs_refused(c, n, bad.data(), stride, 5.0));
    bad = poses;
    for (int q = 3; q < 7; q++) bad[stride + q] = 0.0;   // a zero quaternion
    CHECK(refused(c, n, bad.data(), stride, scoring.data(), 5.0, 0.5, 1) && pairs_refused(c, n, bad.data(), stride, 5.0));
    bad = poses;
    bad[2 * stride] = 1.1e6;   // beyond the coordinate bound: found by the launch, after it wrote device memory
    CHECK(refused(c, n, bad.data(), stride, scoring.data(), 5.0, 0.5, 1) && pairs_refused(c, n, bad.data(), stride, 5.0));
    CHECK(refused(c, n, poses.data(), len - 1, scoring.data(), 5.0, 0.5, 1) && pairs_refused(c, n, poses.data(), len - 1, 5.0));
    CHECK(refused(c, n, nullptr, stride, scoring.data(), 5.0, 0.5, 1) && pairs_refused(c, n, nullptr, stride, 5.0));
    CHECK(refused(nullptr, n, poses.data(), stride, scoring.data(), 5.0, 0.5, 1) && pairs_refused(nullptr, n, poses.data(), stride, 5.0));
    CHECK(refused(c, n, poses.data(), stride, nullptr, 5.0, 0.5, 1));
    const std::vector<double> nan_score = {3.0, NAN, 1.0};
    CHECK(refused(c, n, poses.data(), stride, nan_score.data(), 5.0, 0.5, 1));
    CHECK(refused(c, (size_t)1 << 40, poses.data(), stride, scoring.data(), 5.0, 0.5, 1) && refused(c, 65537, poses.data(), stride, scoring.data(), 5.0, 0.5, 1));
    CHECK(pairs_refused(c, (size_t)1 << 40, poses.data(), stride, 5.0) && pairs_refused(c, ((size_t)1 << 22) + 1, poses.data(), stride, 5.0));
    ld_complex_destroy(c);
}

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: fcc_check <tests/golden> <scratch dir>\n");
        return 2;
    }
    hand_made();
    czy(argv[1]);
    std::printf("fcc_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
