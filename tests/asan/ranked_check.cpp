// ranked_check.cpp -- driver of the sanitizer build around the ranked clustering (`make asan-ranked`;
// tests/test_asan_ranked.py): ld_complex_cluster_ranked through the C ABI against tests/asan/hip_stub.cpp and
// tests/asan/hip_stub_ranked.cpp (device memory = host memory; the ranked launches run their kernels' work in plain C++),
// so the host's checks, sort, sorted upload, round loop and un-permutation run under ASan + UBSan and their outputs are
// compared with a sequential loop written here: 1ppe poses under both measures, n = 0, 1, 64, 65, ties in scoring, and
// every refusal by status with the outputs left as they were.
//   usage: ranked_check <tests/golden> <scratch dir>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
#include <string>
#include <vector>

#define CHECK_PROGRAM "ranked_check"
#include "check.hpp"
#include "kernels/ranked.hpp"
#include "ranked_host.hpp"

struct Side {
    std::vector<double> xyz;
    std::vector<uint32_t> backbone;
    std::string text;   // its ATOM/HETATM lines
};

static Side read_side(const std::string &path, bool keep_backbone = true) {
    Side s;
    std::ifstream in(path);
    std::string line;
    while (std::getline(in, line)) {
        if (line.compare(0, 6, "ATOM  ") != 0 && line.compare(0, 6, "HETATM") != 0) continue;
        std::string name = line.substr(12, 4);
        name.erase(name.find_last_not_of(' ') + 1);
        name.erase(0, name.find_first_not_of(' '));
        const bool bb = name == "CA" || name == "P";
        if (bb && !keep_backbone) continue;
        if (bb) s.backbone.push_back((uint32_t)(s.xyz.size() / 3));
        for (int k = 0; k < 3; k++) s.xyz.push_back(std::strtod(line.substr(30 + 8 * k, 8).c_str(), nullptr));
        s.text += line + "\n";
    }
    return s;
}

struct Result {
    std::vector<int32_t> cluster_of, reps;
    uint32_t n_clusters = 0;
    bool operator==(const Result &o) const { return cluster_of == o.cluster_of && reps == o.reps && n_clusters == o.n_clusters; }
};

// The rule, one pose at a time: (scoring descending, index ascending); the first representative in creation order within
// the cutoff, else a new one.  atoms: the complex atom indices measured.
static Result sequential(const ld::ComplexDevice &m, const std::vector<uint32_t> &atoms, const std::vector<double> &poses, size_t stride,
                         const std::vector<double> &scoring, double cutoff) {
    const size_t n = scoring.size();
    std::vector<std::vector<double>> X(n);
    for (size_t i = 0; i < n; i++)
        for (uint32_t a : atoms) {
            double v[3];
            ranked_host::pose_atom(m, &poses[i * stride], a, v);
            for (int k = 0; k < 3; k++) X[i].push_back(ranked_host::thousandths(v[k]));
        }
    std::vector<size_t> order(n);
    for (size_t i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return scoring[a] > scoring[b]; });
    Result r;
    r.cluster_of.assign(n, -1);
    r.reps.assign(n, -1);
    for (size_t i : order) {
        int32_t joined = -1;
        for (uint32_t c = 0; c < r.n_clusters && joined < 0; c++) {
            double S = 0.0;
            const std::vector<double> &a = X[i], &b = X[(size_t)r.reps[c]];
            for (size_t k = 0; k < a.size(); k++) S += (a[k] - b[k]) * (a[k] - b[k]);
            if (ranked_host::within_cutoff(S, (double)atoms.size(), cutoff)) joined = (int32_t)c;
        }
        if (joined < 0) {
            joined = (int32_t)r.n_clusters;
            r.reps[r.n_clusters++] = (int32_t)i;
        }
        r.cluster_of[i] = joined;
    }
    return r;
}

static Result call(ld_complex *c, const std::vector<double> &poses, size_t stride, const std::vector<double> &scoring, double cutoff,
                   int atoms, int *status) {
    const size_t n = scoring.size();
    Result r;
    r.cluster_of.assign(n, -7);
    r.reps.assign(n, -7);
    r.n_clusters = 12345;
    *status = ld_complex_cluster_ranked(c, n, poses.data(), stride, scoring.data(), cutoff, atoms, r.cluster_of.data(), r.reps.data(),
                                        &r.n_clusters);
    return r;
}

static bool untouched(const Result &r) {
    return r.n_clusters == 12345 && std::all_of(r.cluster_of.begin(), r.cluster_of.end(), [](int32_t v) { return v == -7; }) &&
           std::all_of(r.reps.begin(), r.reps.end(), [](int32_t v) { return v == -7; });
}

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: ranked_check <tests/golden> <scratch dir>\n");
        return 2;
    }
    const std::string golden = argv[1], scratch = argv[2];
    const std::string rec_pdb = golden + "/1ppe/lightdock_1ppe_e.pdb", lig_pdb = golden + "/1ppe/lightdock_1ppe_i.pdb";
    const Side rec = read_side(rec_pdb), lig = read_side(lig_pdb);
    CHECK(!rec.backbone.empty() && !lig.backbone.empty());
    ld::ComplexDevice m;
    m.n_rec = (int)(rec.xyz.size() / 3);
    m.n_lig = (int)(lig.xyz.size() / 3);
    m.rec_xyz = rec.xyz.data();
    m.lig_xyz = lig.xyz.data();
    std::vector<uint32_t> ligand_atoms, complex_atoms = rec.backbone;
    for (uint32_t a : lig.backbone) ligand_atoms.push_back(a + (uint32_t)m.n_rec), complex_atoms.push_back(a + (uint32_t)m.n_rec);

    ld_complex *c = ld_complex_create(rec_pdb.c_str(), lig_pdb.c_str(), nullptr, 0, 0, nullptr, 0, 0);
    CHECK(c != nullptr);
    if (!c) return 1;
    CHECK(ld_complex_pose_len(c) == 7 && ld_complex_num_atoms(c, 2) == complex_atoms.size());

    // poses around a few sites, a stride above the pose length, scores with repeats
    const size_t N = 150, stride = 9;
    std::vector<double> poses(N * stride, std::numeric_limits<double>::quiet_NaN()), scoring(N);   // the padding is never read
    uint64_t seed = 88172645463325252ull;
    auto uniform = [&seed]() {
        seed ^= seed << 13, seed ^= seed >> 7, seed ^= seed << 17;
        return (double)(seed >> 11) / 9007199254740992.0 - 0.5;
    };
    for (size_t i = 0; i < N; i++) {
        double *p = &poses[i * stride];
        const double site = (double)(i % 5) * 9.0;
        for (int k = 0; k < 3; k++) p[k] = site + 6.0 * uniform();
        double q[4] = {1.0, 0.4 * uniform(), 0.4 * uniform(), 0.4 * uniform()};
        const double norm = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        for (int k = 0; k < 4; k++) p[3 + k] = q[k] / norm;
        scoring[i] = std::floor(40.0 * uniform());   // integers: many ties
    }
    auto first = [&](size_t n, std::vector<double> *s) {
        s->assign(scoring.begin(), scoring.begin() + n);
        return std::vector<double>(poses.begin(), poses.begin() + n * stride);
    };

    int status = 0;
    for (int atoms = 0; atoms < 2; atoms++)
        for (double cutoff : {4.0, 1.0, 0.0, 1e9, -1.0})
            for (size_t n : {(size_t)1, (size_t)2, (size_t)63, (size_t)64, (size_t)65, N}) {
                std::vector<double> s;
                const std::vector<double> p = first(n, &s);
                const Result got = call(c, p, stride, s, cutoff, atoms, &status);
                CHECK(status == LD_OK);
                const Result want = sequential(m, atoms ? ligand_atoms : complex_atoms, p, stride, s, cutoff);
                CHECK(got == want);
                if (cutoff == 1e9) CHECK(got.n_clusters == 1);
                if (cutoff <= 0.0) CHECK(got.n_clusters == n);
            }
    {   // all scores equal: index order
        std::vector<double> s;
        const std::vector<double> p = first(N, &s);
        std::fill(s.begin(), s.end(), 2.5);
        const Result got = call(c, p, stride, s, 0.0, 1, &status);
        CHECK(status == LD_OK && got.n_clusters == N);
        for (size_t i = 0; i < N; i++) CHECK(got.reps[i] == (int32_t)i && got.cluster_of[i] == (int32_t)i);
        CHECK(call(c, p, stride, s, 4.0, 0, &status) == sequential(m, complex_atoms, p, stride, s, 4.0));
    }
    {   // n = 0: LD_OK, one word written, nothing else asked for
        uint32_t count = 99;
        CHECK(ld_complex_cluster_ranked(c, 0, nullptr, 7, nullptr, 4.0, 0, nullptr, nullptr, &count) == LD_OK && count == 0);
    }
    double ms = -1.0;
    CHECK(ld_complex_last_kernel_ms(c, &ms) == LD_OK && ms >= 0.0);

    // refusals: status, a message, the outputs as they were
    {
        std::vector<double> s;
        const std::vector<double> p = first(8, &s);
        auto refused = [&](const std::vector<double> &pp, size_t st, const std::vector<double> &ss, double cutoff, int atoms) {
            const Result r = call(c, pp, st, ss, cutoff, atoms, &status);
            CHECK(status == LD_ERR_INVALID && std::strlen(ld_last_error()) > 0 && untouched(r));
        };
        refused(p, stride, s, std::numeric_limits<double>::quiet_NaN(), 0);
        refused(p, stride, s, 4.0, 2);
        refused(p, stride, s, 4.0, -1);
        refused(p, 6, s, 4.0, 0);   // stride below the pose length
        for (double bad : {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity()}) {
            std::vector<double> sb = s, pb = p;
            sb[5] = bad;
            refused(p, stride, sb, 4.0, 0);
            pb[3 * stride + 4] = bad;
            refused(pb, stride, s, 4.0, 1);
        }
        std::vector<double> zero = p;
        for (int k = 3; k < 7; k++) zero[2 * stride + k] = 0.0;
        refused(zero, stride, s, 4.0, 0);
        std::vector<double> far = p;
        far[7 * stride + 1] = 3.0e6;   // 3e9 thousandths: beyond an int32
        refused(far, stride, s, 4.0, 0);
        refused(far, stride, s, 4.0, 1);
        // the workspace bound, from arithmetic alone: the list is never read
        const size_t per_pose = ligand_atoms.size() * 12, too_many = ld::kRankedWorkspaceBytes / per_pose + 1;
        Result r;
        r.cluster_of.assign(8, -7), r.reps.assign(8, -7), r.n_clusters = 12345;
        CHECK(ld_complex_cluster_ranked(c, too_many, p.data(), stride, s.data(), 4.0, 1, r.cluster_of.data(), r.reps.data(), &r.n_clusters) ==
              LD_ERR_INVALID);
        CHECK(untouched(r));
        CHECK(ld_complex_cluster_ranked(c, too_many, p.data(), stride, s.data(), 4.0, 0, r.cluster_of.data(), r.reps.data(), &r.n_clusters) ==
              LD_ERR_INVALID);   // rigid receptor: the same walk
        CHECK(ld_complex_cluster_ranked(c, (size_t)-1, p.data(), stride, s.data(), 4.0, 0, r.cluster_of.data(), r.reps.data(), &r.n_clusters) ==
              LD_ERR_INVALID);
        CHECK(untouched(r));
        // null arguments
        CHECK(ld_complex_cluster_ranked(nullptr, 8, p.data(), stride, s.data(), 4.0, 0, r.cluster_of.data(), r.reps.data(), &r.n_clusters) == LD_ERR_INVALID);
        CHECK(ld_complex_cluster_ranked(c, 8, nullptr, stride, s.data(), 4.0, 0, r.cluster_of.data(), r.reps.data(), &r.n_clusters) == LD_ERR_INVALID);
        CHECK(ld_complex_cluster_ranked(c, 8, p.data(), stride, nullptr, 4.0, 0, r.cluster_of.data(), r.reps.data(), &r.n_clusters) == LD_ERR_INVALID);
        CHECK(ld_complex_cluster_ranked(c, 8, p.data(), stride, s.data(), 4.0, 0, nullptr, r.reps.data(), &r.n_clusters) == LD_ERR_INVALID);
        CHECK(ld_complex_cluster_ranked(c, 8, p.data(), stride, s.data(), 4.0, 0, r.cluster_of.data(), nullptr, &r.n_clusters) == LD_ERR_INVALID);
        CHECK(ld_complex_cluster_ranked(c, 8, p.data(), stride, s.data(), 4.0, 0, r.cluster_of.data(), r.reps.data(), nullptr) == LD_ERR_INVALID);
        CHECK(untouched(r));
        // and the complex still serves
        CHECK(call(c, p, stride, s, 4.0, 0, &status) == sequential(m, complex_atoms, p, stride, s, 4.0) && status == LD_OK);
    }
    ld_complex_destroy(c);

    // no CA / P atom in the chosen set: a ligand without one is refused under atoms = 1 only; a complex without one always
    {
        const std::string bare_lig = scratch + "/ligand_without_ca.pdb", bare_rec = scratch + "/receptor_without_ca.pdb";
        const Side lig_bare = read_side(lig_pdb, false), rec_bare = read_side(rec_pdb, false);
        put(bare_lig, lig_bare.text);
        put(bare_rec, rec_bare.text);
        std::vector<double> s;
        const std::vector<double> p = first(70, &s);
        ld_complex *half = ld_complex_create(rec_pdb.c_str(), bare_lig.c_str(), nullptr, 0, 0, nullptr, 0, 0);
        CHECK(half != nullptr);
        if (half) {
            Result r = call(half, p, stride, s, 4.0, 1, &status);
            CHECK(status == LD_ERR_INVALID && untouched(r));
            // atoms = 0: the receptor's CA atoms are all there is, and none of them moves: one cluster
            r = call(half, p, stride, s, 4.0, 0, &status);
            CHECK(status == LD_OK && r.n_clusters == 1);
            ld::ComplexDevice hm = m;
            hm.n_lig = (int)(lig_bare.xyz.size() / 3);
            hm.lig_xyz = lig_bare.xyz.data();
            CHECK(r == sequential(hm, rec.backbone, p, stride, s, 4.0));
            ld_complex_destroy(half);
        }
        ld_complex *none = ld_complex_create(bare_rec.c_str(), bare_lig.c_str(), nullptr, 0, 0, nullptr, 0, 0);
        CHECK(none != nullptr);
        if (none) {
            for (int atoms = 0; atoms < 2; atoms++) {
                const Result r = call(none, p, stride, s, 4.0, atoms, &status);
                CHECK(status == LD_ERR_INVALID && untouched(r));
            }
            ld_complex_destroy(none);
        }
    }
    std::printf("ranked_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
