// ccs_check.cpp -- driver of the sanitizer build of the collision cross-section path (`make asan-ccs`;
// tests/test_asan_ccs.py): ld_ccs_frames / ld_complex_ccs through the C ABI against tests/asan/hip_stub.cpp and
// tests/asan/hip_stub_ccs.cpp (device memory = host memory; the launches do the kernels' work in plain C++ from the shared
// rule, so the answers are real ones): one- and two-atom cases whose counts the rule's text pins, three 1czy poses in all
// three selections, the rigid-receptor form against the plain one, more poses than workspace slots, every NULL / non-NULL
// combination of the outputs, and every refusal by status with the outputs untouched.
//   usage: ccs_check <tests/golden> <scratch dir>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#define CHECK_PROGRAM "ccs_check"
#include "check.hpp"
#include "host/io.hpp"

static const size_t V = LD_CCS_VIEWS;

// The columns after the coordinates up to the element (77-78) and the line end.
static std::string rest(const char *element) {
    char buf[64];
    std::snprintf(buf, sizeof buf, "  1.00  0.00          %2s  \n", element);
    return buf;
}

static ld_complex *two_files(const std::string &scratch, const char *tag, const std::string &rec, const std::string &lig) {
    const std::string r = scratch + "/" + tag + "_rec.pdb", l = scratch + "/" + tag + "_lig.pdb";
    put(r, rec);
    put(l, lig);
    return ld_complex_create(r.c_str(), l.c_str(), nullptr, 0, 0, nullptr, 0, 0);
}

struct Out {
    std::vector<uint32_t> counts;
    std::vector<uint64_t> sums;
    explicit Out(size_t n) : counts(n * V, 0xA5A5A5A5u), sums(n, 0xA5A5A5A5A5A5A5A5ull) {}
    bool untouched() const {
        for (uint32_t v : counts)
            if (v != 0xA5A5A5A5u) return false;
        for (uint64_t v : sums)
            if (v != 0xA5A5A5A5A5A5A5A5ull) return false;
        return true;
    }
    bool sums_are_of_counts() const {
        for (size_t i = 0; i < sums.size(); i++) {
            uint64_t s = 0;
            for (size_t v = 0; v < V; v++) s += counts[i * V + v];
            if (s != sums[i]) return false;
        }
        return true;
    }
};

static std::vector<double> rigid(const std::vector<double> &tx, double ty = 0.0) {
    std::vector<double> poses(tx.size() * 7, 0.0);
    for (size_t i = 0; i < tx.size(); i++) poses[i * 7] = tx[i], poses[i * 7 + 1] = ty, poses[i * 7 + 3] = 1.0;
    return poses;
}

static void tiny(const std::string &scratch) {
    int32_t F[LD_CCS_VIEWS * 6];
    CHECK(ld_ccs_frames(F) == LD_OK && ld_ccs_frames(nullptr) == LD_ERR_INVALID);
    CHECK(F[0] == 0 && F[1] == 1048576 && F[2] == 0 && F[3] == -1040384 && F[4] == 0 && F[5] == 130816 && F[6] == -708303 && F[11] == 225689);

    // two carbons, one a molecule; a hydrogen of the receptor and a bead of the ligand take no part
    ld_complex *c = two_files(scratch, "cc", atom_line(1, "C", "GLY", 'A', 1, 0, 0, 0, rest("C").c_str()) + atom_line(2, "H", "GLY", 'A', 1, 9, 0, 0, rest("H").c_str()),
                              atom_line(1, "BJ", "MMB", 'B', 1, -9, 0, 0, rest("C").c_str()) + atom_line(2, "C", "GLY", 'B', 2, 0, 0, 0, rest("C").c_str()));
    CHECK(c != nullptr);
    if (!c) return;
    // an atom at the origin projects to (0, 0) in every view: E = 2500 at h = 500 covers 81 points, 12 of them on the rim
    const std::vector<double> tx = {0.0, 4000.0, -4000.0, 2.0, -1.9995};
    const std::vector<double> poses = rigid(tx);
    Out rec(tx.size()), lig(tx.size()), both(tx.size());
    CHECK(ld_complex_ccs(c, tx.size(), poses.data(), 7, 0, 0.8, 0.5, rec.counts.data(), rec.sums.data()) == LD_OK);
    CHECK(ld_complex_ccs(c, tx.size(), poses.data(), 7, 1, 0.8, 0.5, lig.counts.data(), lig.sums.data()) == LD_OK);
    CHECK(ld_complex_ccs(c, tx.size(), poses.data(), 7, 2, 0.8, 0.5, both.counts.data(), both.sums.data()) == LD_OK);
    CHECK(rec.sums_are_of_counts() && lig.sums_are_of_counts() && both.sums_are_of_counts());
    for (size_t i = 0; i < tx.size(); i++)
        for (size_t v = 0; v < V; v++) {
            const uint32_t r = rec.counts[i * V + v], l = lig.counts[i * V + v], b = both.counts[i * V + v];
            CHECK(r == 81);
            if (i == 0) CHECK(l == 81 && b == 81);        // coincident: the count of one
            if (i == 1 || i == 2) CHECK(b == r + l);      // far apart: the sum
            if (i >= 3) CHECK(b >= r && b >= l && b <= r + l);
        }
    Out edge(1);
    CHECK(ld_complex_ccs(c, 1, poses.data(), 7, 0, 0.799, 0.5, edge.counts.data(), nullptr) == LD_OK && edge.counts[0] == 69 && edge.counts[63] == 69);
    CHECK(ld_complex_ccs(c, 1, poses.data(), 7, 0, 1.0, 2.0, edge.counts.data(), edge.sums.data()) == LD_OK && edge.counts[17] == 5 && edge.sums[0] == 5 * V);   // i^2 + j^2 <= 1.35^2
    CHECK(ld_complex_ccs(c, 1, poses.data(), 7, 0, 0.0, 0.1, edge.counts.data(), edge.sums.data()) == LD_OK && edge.counts[5] == 901);   // i^2 + j^2 <= 17^2

    // long thin boxes at the finest lattice, inside the bound; a box beyond it is refused with nothing written
    const std::vector<double> far = rigid({1500.0}, 1500.0), beyond = rigid({1700.0}, 1700.0);
    Out thin(1), none(1);
    CHECK(ld_complex_ccs(c, 1, far.data(), 7, 2, 1.0, 0.1, thin.counts.data(), thin.sums.data()) == LD_OK && thin.sums_are_of_counts());
    CHECK(ld_complex_ccs(c, 1, far.data(), 7, 0, 1.0, 0.1, none.counts.data(), none.sums.data()) == LD_OK && thin.counts[0] > none.counts[0]);
    none = Out(1);
    CHECK(ld_complex_ccs(c, 1, beyond.data(), 7, 2, 1.0, 0.1, none.counts.data(), none.sums.data()) == LD_ERR_INVALID && none.untouched());
    CHECK(ld_complex_ccs(c, 1, beyond.data(), 7, 1, 1.0, 0.1, none.counts.data(), none.sums.data()) == LD_OK);   // the ligand alone: a small box
    ld_complex_destroy(c);

    // a ligand of which no atom takes part: the ligand alone is refused, the receptor and the complex are measured
    c = two_files(scratch, "hh", atom_line(1, "C", "GLY", 'A', 1, 0, 0, 0, rest("C").c_str()),
                  atom_line(1, "H", "GLY", 'B', 1, 0, 0, 0, rest("H").c_str()) + atom_line(2, "BJ", "MMB", 'B', 2, 1, 0, 0, rest("C").c_str()));
    CHECK(c != nullptr);
    if (!c) return;
    Out h(1);
    CHECK(ld_complex_ccs(c, 1, poses.data(), 7, 1, 1.0, 0.5, h.counts.data(), h.sums.data()) == LD_ERR_INVALID && h.untouched());
    CHECK(ld_complex_ccs(c, 1, poses.data(), 7, 2, 0.8, 0.5, h.counts.data(), h.sums.data()) == LD_OK && h.sums[0] == 81 * V);
    CHECK(ld_complex_ccs(c, 1, poses.data(), 7, 0, 0.8, 0.5, h.counts.data(), h.sums.data()) == LD_OK && h.sums[0] == 81 * V);
    ld_complex_destroy(c);
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
    const std::string rec = d + "lightdock_1czy_protein.pdb", lig = d + "lightdock_1czy_peptide.pdb";
    ld_complex *c = ld_complex_create(rec.c_str(), lig.c_str(), rec_nm.data(), rec_nm.size(), 10, lig_nm.data(), lig_nm.size(), 10);
    ld_complex *r = ld_complex_create(rec.c_str(), lig.c_str(), nullptr, 0, 0, nullptr, 0, 0);
    CHECK(c != nullptr && r != nullptr);
    if (!c || !r) return;
    const size_t len = ld_complex_pose_len(c);
    CHECK(len == 27 && ld_complex_pose_len(r) == 7);
    const size_t stride = len + 2, n = 3;
    std::vector<double> poses(n * stride, 0.0);
    const std::vector<double> first = gso_pose(d + "swarm_2/gso_100.out", 74), second = gso_pose(d + "swarm_0/gso_100.out", 0),
                              third = gso_pose(d + "swarm_9/gso_100.out", 199);
    CHECK(first.size() == 27 && second.size() == 27 && third.size() == 27);
    if (first.size() != 27 || second.size() != 27 || third.size() != 27) return;
    std::copy(first.begin(), first.end(), poses.begin());
    std::copy(second.begin(), second.end(), poses.begin() + stride);
    std::copy(third.begin(), third.end(), poses.begin() + 2 * stride);
    Out o[3] = {Out(n), Out(n), Out(n)};
    for (int what = 0; what < 3; what++) {
        CHECK(ld_complex_ccs(c, n, poses.data(), stride, what, 1.0, 0.5, o[what].counts.data(), o[what].sums.data()) == LD_OK);
        CHECK(o[what].sums_are_of_counts());
    }
    bool ordered = true;
    for (size_t k = 0; k < n * V; k++)
        ordered = ordered && o[2].counts[k] >= o[0].counts[k] && o[2].counts[k] >= o[1].counts[k] && o[2].counts[k] <= o[0].counts[k] + o[1].counts[k] && o[1].counts[k] > 0;
    CHECK(ordered);
    // every NULL / non-NULL combination gives the same numbers
    for (int mask = 0; mask < 4; mask++) {
        Out p(n);
        CHECK(ld_complex_ccs(c, n, poses.data(), stride, 2, 1.0, 0.5, mask & 1 ? p.counts.data() : nullptr, mask & 2 ? p.sums.data() : nullptr) == LD_OK);
        CHECK(!(mask & 1) || p.counts == o[2].counts);
        CHECK(!(mask & 2) || p.sums == o[2].sums);
        if (mask == 0) CHECK(p.untouched());
    }
    double ms = -1.0;
    CHECK(ld_complex_last_kernel_ms(c, &ms) == LD_OK && ms == 0.0);
    CHECK(ld_complex_ccs(c, 0, nullptr, len, 2, 1.0, 0.5, nullptr, nullptr) == LD_OK);

    // the rigid-receptor form (no modes) and the plain form (modes, at zero extents) give the same bits
    std::vector<double> flat(n * stride, 0.0);
    for (size_t i = 0; i < n; i++) std::copy(poses.begin() + i * stride, poses.begin() + i * stride + 7, flat.begin() + i * stride);
    Out plain(n), fast(n);
    CHECK(ld_complex_ccs(c, n, flat.data(), stride, 2, 1.0, 0.5, plain.counts.data(), plain.sums.data()) == LD_OK);
    CHECK(ld_complex_ccs(r, n, flat.data(), stride, 2, 1.0, 0.5, fast.counts.data(), fast.sums.data()) == LD_OK);
    CHECK(plain.counts == fast.counts && plain.sums == fast.sums && plain.counts != o[2].counts);
    CHECK(ld_complex_ccs(r, 1, flat.data(), stride, 2, 1.4, 1.0, fast.counts.data(), nullptr) == LD_OK);
    CHECK(ld_complex_ccs(c, 1, flat.data(), stride, 2, 1.4, 1.0, plain.counts.data(), nullptr) == LD_OK && plain.counts == fast.counts);

    // refusals: nothing written
    for (ld_complex *x : {c, r}) {
        const std::vector<double> &good = x == c ? poses : flat;
        Out q(n);
        auto refused = [&](const double *p, size_t st, int what, double probe, double cell) {
            return ld_complex_ccs(x, n, p, st, what, probe, cell, q.counts.data(), q.sums.data()) == LD_ERR_INVALID && q.untouched();
        };
        for (double probe : {-0.001, -1.0, 2.001, (double)NAN, (double)INFINITY, -(double)INFINITY, 1e300}) CHECK(refused(good.data(), stride, 2, probe, 0.5));
        for (double cell : {0.0994, 0.0, -0.5, 2.0006, (double)NAN, (double)INFINITY, -(double)INFINITY, 1e300}) CHECK(refused(good.data(), stride, 2, 1.0, cell));
        for (int what : {-1, 3, 1 << 20}) CHECK(refused(good.data(), stride, what, 1.0, 0.5));
        std::vector<double> bad = good;
        bad[stride + 5] = NAN;
        CHECK(refused(bad.data(), stride, 2, 1.0, 0.5));
        bad = good;
        bad[2 * stride + 1] = INFINITY;
        CHECK(refused(bad.data(), stride, 1, 1.0, 0.5));
        bad = good;
        for (int k = 3; k < 7; k++) bad[stride + k] = 0.0;   // a zero quaternion
        CHECK(refused(bad.data(), stride, 2, 1.0, 0.5));
        CHECK(refused(good.data(), ld_complex_pose_len(x) - 1, 2, 1.0, 0.5) && refused(nullptr, stride, 2, 1.0, 0.5));
        bad = good;
        bad[2 * stride] = 1.1e6;   // beyond the coordinate bound: found by the launch, after it wrote device memory
        CHECK(refused(bad.data(), stride, 2, 1.0, 0.5) && refused(bad.data(), stride, 1, 1.0, 0.5));
        CHECK(ld_complex_ccs(x, n, bad.data(), stride, 0, 1.0, 0.5, q.counts.data(), q.sums.data()) == LD_OK);   // the receptor alone does not move
        bad[2 * stride] = 3000.0;   // 3000 A away at h = 500: a box of 6000 x 6000 points at most, inside the bound
        CHECK(ld_complex_ccs(x, n, bad.data(), stride, 2, 1.0, 0.5, q.counts.data(), q.sums.data()) == LD_OK && q.sums_are_of_counts());
        bad[2 * stride] = 0.9e6;    // inside the coordinate bound, beyond the box bound
        CHECK(ld_complex_ccs(x, n, bad.data(), stride, 2, 1.0, 0.5, nullptr, nullptr) == LD_ERR_INVALID);
    }
    CHECK(ld_complex_ccs(nullptr, n, poses.data(), stride, 2, 1.0, 0.5, nullptr, nullptr) == LD_ERR_INVALID);
    ld_complex_destroy(c);
    ld_complex_destroy(r);
}

// More poses than workspace slots, on a small complex.
static void many(const std::string &scratch) {
    ld_complex *c = two_files(scratch, "many", atom_line(1, "N", "GLY", 'A', 1, 0, 0, 0, rest("N").c_str()) + atom_line(2, "CA", "GLY", 'A', 1, 1.5, 0, 0, rest("C").c_str()),
                              atom_line(1, "P", "DT", 'B', 1, 0, 0, 0, rest("P").c_str()));
    CHECK(c != nullptr);
    if (!c) return;
    const size_t n = 1500;
    std::vector<double> tx(n);
    for (size_t i = 0; i < n; i++) tx[i] = 0.004 * (double)(i % 750);
    const std::vector<double> poses = rigid(tx);
    Out o(n);
    CHECK(ld_complex_ccs(c, n, poses.data(), 7, 2, 1.0, 0.5, o.counts.data(), o.sums.data()) == LD_OK && o.sums_are_of_counts());
    bool same = true;
    for (size_t i = 0; i < 750; i++) same = same && o.sums[i] == o.sums[i + 750] && std::memcmp(&o.counts[i * V], &o.counts[(i + 750) * V], V * sizeof(uint32_t)) == 0;
    CHECK(same && o.sums[0] != o.sums[749]);
    ld_complex_destroy(c);
}

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: ccs_check <tests/golden> <scratch dir>\n");
        return 2;
    }
    tiny(argv[2]);
    czy(argv[1]);
    many(argv[2]);
    std::printf("ccs_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
