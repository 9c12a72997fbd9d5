// xlink_check.cpp -- driver of the sanitizer build of the cross-link path (`make asan-xlinks`; tests/test_asan_xlinks.py):
// ld_complex_crosslinks through the C ABI against tests/asan/hip_stub.cpp and tests/asan/hip_stub_xlink.cpp (device memory =
// host memory; the launches do the kernels' work in plain C++ from the shared rule, so the answers are real ones): one- and
// two-atom cases whose distances the rule's text pins, three 1czy poses, more jobs than workspace slots, every NULL /
// non-NULL combination of the outputs, and every refusal by status with the outputs untouched.
//   usage: xlink_check <tests/golden> <scratch dir>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#define CHECK_PROGRAM "xlink_check"
#include "check.hpp"
#include "host/io.hpp"

static const uint32_t NONE = LD_XLINK_NO_PATH;

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
    std::vector<uint64_t> straight2;
    std::vector<uint32_t> path;
    Out(size_t n, size_t L) : straight2(n * L, 0xA5A5A5A5A5A5A5A5ull), path(n * L, 0xA5A5A5A5u) {}
    bool untouched() const {
        for (uint64_t v : straight2)
            if (v != 0xA5A5A5A5A5A5A5A5ull) return false;
        for (uint32_t v : path)
            if (v != 0xA5A5A5A5u) return false;
        return true;
    }
};

static std::vector<double> rigid(const std::vector<double> &tx) {
    std::vector<double> poses(tx.size() * 7, 0.0);
    for (size_t i = 0; i < tx.size(); i++) poses[i * 7] = tx[i], poses[i * 7 + 3] = 1.0;
    return poses;
}

static int run(ld_complex *c, size_t n, const std::vector<double> &poses, const std::vector<uint32_t> &links, Out &o, double probe = 0.0,
               double cell = 1.0, double reach = 3.0, double max_length = 12.0) {
    return ld_complex_crosslinks(c, n, poses.data(), poses.size() / (n ? n : 1), links.size() / 2, links.data(), probe, cell, reach, max_length,
                                 o.straight2.data(), o.path.data());
}

static void tiny(const std::string &scratch) {
    // a carbon a molecule; a hydrogen of the receptor takes no part and may still be an anchor
    ld_complex *c = two_files(scratch, "cc", atom_line(1, "C", "GLY", 'A', 1, 0, 0, 0, rest("C").c_str()) + atom_line(2, "H", "GLY", 'A', 1, 0, 5, 0, rest("H").c_str()),
                              atom_line(1, "C", "GLY", 'B', 1, 0, 0, 0, rest("C").c_str()));
    CHECK(c != nullptr);
    if (!c) return;
    const std::vector<double> poses = rigid({10.0, -10.0, 10.0005, 40.0});
    const std::vector<uint32_t> links = {0, 2, 2, 0, 0, 0, 1, 1, 0, 1};
    Out o(4, 5);
    CHECK(run(c, 4, poses, links, o) == LD_OK);
    // along the axis: the doors (2, 0, 0) and (8, 0, 0), hops of 2000 and six moves of 1000 -- the straight distance itself
    CHECK(o.straight2[0] == 100000000ull && o.path[0] == 10000 && o.path[1] == 10000 && o.straight2[1] == 100000000ull);
    CHECK(o.straight2[5] == 100000000ull && o.path[5] == 10000);
    // the nearest free node of a lone carbon (R = 1700) is (1, 1, 1): a hop of isqrt(3 000 000) = 1732 there and back
    CHECK(o.straight2[2] == 0 && o.path[2] == 2 * 1732);
    // the hydrogen, at a free node: no hop at all
    CHECK(o.straight2[3] == 0 && o.path[3] == 0 && o.straight2[4] == 25000000ull);
    CHECK(o.straight2[10] == 10001ull * 10001ull || o.straight2[10] == 10000ull * 10000ull);   // 10.0005 prints as one of the two
    CHECK(o.straight2[15] == 1600000000ull && o.path[15] == NONE && o.path[17] == 2 * 1732);   // 40 A apart, M = 12 A
    // a reach of 1 A finds no free node about a carbon: no path, the straight distance all the same
    Out none(4, 5);
    CHECK(run(c, 4, poses, links, none, 0.0, 1.0, 1.0) == LD_OK && none.path[0] == NONE && none.path[2] == NONE && none.straight2[0] == 100000000ull);
    CHECK(none.path[3] == 0);   // the hydrogen is its own door
    // D == M is reported, D == M + 1 is not
    Out edge(4, 5);
    CHECK(run(c, 4, poses, links, edge, 0.0, 1.0, 3.0, 10.0) == LD_OK && edge.path[0] == 10000);
    CHECK(run(c, 4, poses, links, edge, 0.0, 1.0, 3.0, 9.999) == LD_OK && edge.path[0] == NONE && edge.path[2] == 2 * 1732);
    // other cells and a probe
    for (double cell : {0.5, 2.0})
        for (double probe : {0.0, 1.4}) {
            Out p(4, 5);
            CHECK(run(c, 4, poses, links, p, probe, cell, 4.0, 14.0) == LD_OK && p.path[0] == p.path[1] && p.path[0] == p.path[5] && p.path[0] >= 9990 && p.path[0] <= 14000);
        }
    ld_complex_destroy(c);

    // a complex of which no atom takes part: straight distances only
    c = two_files(scratch, "hh", atom_line(1, "H", "GLY", 'A', 1, 0, 0, 0, rest("H").c_str()), atom_line(1, "BJ", "MMB", 'B', 1, 1, 0, 0, rest("C").c_str()));
    CHECK(c != nullptr);
    if (!c) return;
    const std::vector<uint32_t> one = {0, 1};
    Out h(4, 1);
    CHECK(run(c, 4, poses, one, h) == LD_ERR_INVALID && h.untouched());
    CHECK(ld_complex_crosslinks(c, 4, poses.data(), 7, 1, one.data(), 0.0, 1.0, 3.0, 12.0, h.straight2.data(), nullptr) == LD_OK && h.straight2[0] == 121000000ull);
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
    CHECK(c != nullptr);
    if (!c) return;
    const size_t len = ld_complex_pose_len(c), n_rec = ld_complex_num_atoms(c, 0), n_all = n_rec + ld_complex_num_atoms(c, 1);
    CHECK(len == 27 && n_rec > 400 && n_all > n_rec + 10);
    const size_t stride = len + 2, n = 3;
    std::vector<double> poses(n * stride, 0.0);
    const std::vector<double> first = gso_pose(d + "swarm_2/gso_100.out", 74), second = gso_pose(d + "swarm_0/gso_100.out", 0),
                              third = gso_pose(d + "swarm_9/gso_100.out", 199);
    CHECK(first.size() == 27 && second.size() == 27 && third.size() == 27);
    if (first.size() != 27 || second.size() != 27 || third.size() != 27) return;
    std::copy(first.begin(), first.end(), poses.begin());
    std::copy(second.begin(), second.end(), poses.begin() + stride);
    std::copy(third.begin(), third.end(), poses.begin() + 2 * stride);
    const uint32_t R = (uint32_t)n_rec;
    const std::vector<uint32_t> links = {0, R + 5, 100, 200, 100, R + 1, 50, 50, R + 1, R + 9, 200, 100, 7, 100};
    const size_t L = links.size() / 2;
    Out o(n, L);
    CHECK(run(c, n, poses, links, o) == LD_OK);
    bool sane = true, some = false;
    for (size_t i = 0; i < n; i++) {
        sane = sane && o.path[i * L + 1] == o.path[i * L + 5] && o.straight2[i * L + 1] == o.straight2[i * L + 5] && o.straight2[i * L + 3] == 0;
        for (size_t l = 0; l < L; l++) {
            const uint32_t p = o.path[i * L + l];
            some = some || p != NONE;
            // a path is no shorter than the straight line, less the floors of its hops and moves
            sane = sane && (p == NONE || (p <= 12000 && ((uint64_t)p + 16) * ((uint64_t)p + 16) >= o.straight2[i * L + l]));
        }
    }
    CHECK(sane && some);
    // every NULL / non-NULL combination gives the same numbers
    for (int mask = 0; mask < 4; mask++) {
        Out p(n, L);
        CHECK(ld_complex_crosslinks(c, n, poses.data(), stride, L, links.data(), 0.0, 1.0, 3.0, 12.0, mask & 1 ? p.straight2.data() : nullptr,
                                    mask & 2 ? p.path.data() : nullptr) == LD_OK);
        CHECK(!(mask & 1) || p.straight2 == o.straight2);
        CHECK(!(mask & 2) || p.path == o.path);
        if (mask == 0) CHECK(p.untouched());
    }
    double ms = -1.0;
    CHECK(ld_complex_last_kernel_ms(c, &ms) == LD_OK && ms == 0.0);
    CHECK(ld_complex_crosslinks(c, 0, nullptr, len, L, links.data(), 0.0, 1.0, 3.0, 12.0, nullptr, nullptr) == LD_OK);
    // the links reversed and repeated: the same words at their places
    std::vector<uint32_t> again;
    for (size_t l = L; l-- > 0;) again.push_back(links[2 * l + 1]), again.push_back(links[2 * l]);
    again.insert(again.end(), links.begin(), links.end());
    Out q(n, 2 * L);
    CHECK(run(c, n, poses, again, q) == LD_OK);
    bool same = true;
    for (size_t i = 0; i < n; i++)
        for (size_t l = 0; l < L; l++)
            same = same && q.path[i * 2 * L + (L - 1 - l)] == o.path[i * L + l] && q.path[i * 2 * L + L + l] == o.path[i * L + l] &&
                   q.straight2[i * 2 * L + (L - 1 - l)] == o.straight2[i * L + l];
    CHECK(same);

    // refusals: nothing written
    Out r(n, L);
    auto refused = [&](const double *p, size_t st, size_t n_links, const uint32_t *lk, double probe, double cell, double reach, double max_length) {
        return ld_complex_crosslinks(c, n, p, st, n_links, lk, probe, cell, reach, max_length, r.straight2.data(), r.path.data()) == LD_ERR_INVALID && r.untouched();
    };
    const double nan = NAN, inf = INFINITY;
    for (double probe : {-0.001, -1.0, 2.001, nan, inf, -inf, 1e300}) CHECK(refused(poses.data(), stride, L, links.data(), probe, 1.0, 3.0, 12.0));
    for (double cell : {0.4994, 0.0, -1.0, 2.0006, nan, inf, -inf, 1e300}) CHECK(refused(poses.data(), stride, L, links.data(), 0.0, cell, 3.0, 12.0));
    for (double reach : {0.0004, 0.0, -1.0, 6.0006, nan, inf, -inf, 1e300}) CHECK(refused(poses.data(), stride, L, links.data(), 0.0, 1.0, reach, 12.0));
    for (double max_length : {0.9994, 0.0, -1.0, 60.0006, nan, inf, -inf, 1e300}) CHECK(refused(poses.data(), stride, L, links.data(), 0.0, 1.0, 3.0, max_length));
    CHECK(refused(poses.data(), stride, L, links.data(), 0.0, 0.5, 3.0, 40.5));   // 81 cells
    CHECK(refused(poses.data(), stride, 0, links.data(), 0.0, 1.0, 3.0, 12.0) && refused(poses.data(), stride, 4097, links.data(), 0.0, 1.0, 3.0, 12.0));
    CHECK(refused(poses.data(), stride, L, nullptr, 0.0, 1.0, 3.0, 12.0));
    std::vector<uint32_t> beyond = links;
    beyond[5] = (uint32_t)n_all;
    CHECK(refused(poses.data(), stride, L, beyond.data(), 0.0, 1.0, 3.0, 12.0));
    beyond[5] = 0xFFFFFFFFu;
    CHECK(refused(poses.data(), stride, L, beyond.data(), 0.0, 1.0, 3.0, 12.0));
    std::vector<double> bad = poses;
    bad[stride + 5] = NAN;
    CHECK(refused(bad.data(), stride, L, links.data(), 0.0, 1.0, 3.0, 12.0));
    bad = poses;
    bad[2 * stride + 1] = INFINITY;
    CHECK(refused(bad.data(), stride, L, links.data(), 0.0, 1.0, 3.0, 12.0));
    bad = poses;
    for (int k = 3; k < 7; k++) bad[stride + k] = 0.0;   // a zero quaternion
    CHECK(refused(bad.data(), stride, L, links.data(), 0.0, 1.0, 3.0, 12.0));
    CHECK(refused(poses.data(), len - 1, L, links.data(), 0.0, 1.0, 3.0, 12.0) && refused(nullptr, stride, L, links.data(), 0.0, 1.0, 3.0, 12.0));
    bad = poses;
    bad[2 * stride] = 1.1e6;   // beyond the coordinate bound: found by the launch, after it wrote device memory
    CHECK(refused(bad.data(), stride, L, links.data(), 0.0, 1.0, 3.0, 12.0));
    // ... a ligand blocker beyond it refuses the paths of receptor links, not their straight distances
    const std::vector<uint32_t> inner = {100, 200};
    CHECK(ld_complex_crosslinks(c, n, bad.data(), stride, 1, inner.data(), 0.0, 1.0, 3.0, 12.0, r.straight2.data(), nullptr) == LD_OK);
    r = Out(n, L);
    CHECK(ld_complex_crosslinks(c, n, bad.data(), stride, 1, inner.data(), 0.0, 1.0, 3.0, 12.0, r.straight2.data(), r.path.data()) == LD_ERR_INVALID && r.untouched());
    CHECK(ld_complex_crosslinks(nullptr, n, poses.data(), stride, L, links.data(), 0.0, 1.0, 3.0, 12.0, nullptr, nullptr) == LD_ERR_INVALID);
    ld_complex_destroy(c);
}

// More jobs than workspace slots, on a small complex.
static void many(const std::string &scratch) {
    ld_complex *c = two_files(scratch, "many", atom_line(1, "N", "GLY", 'A', 1, 0, 0, 0, rest("N").c_str()) + atom_line(2, "CA", "GLY", 'A', 1, 1.5, 0, 0, rest("C").c_str()),
                              atom_line(1, "P", "DT", 'B', 1, 0, 0, 0, rest("P").c_str()));
    CHECK(c != nullptr);
    if (!c) return;
    const size_t n = 700;
    std::vector<double> tx(n);
    for (size_t i = 0; i < n; i++) tx[i] = 4.0 + 0.004 * (double)(i % 350);
    const std::vector<double> poses = rigid(tx);
    const std::vector<uint32_t> links = {0, 2, 1, 2};
    Out o(n, 2);
    CHECK(run(c, n, poses, links, o, 0.0, 1.0, 3.0, 6.0) == LD_OK);
    bool same = true, moved = false;
    for (size_t i = 0; i < 350; i++) {
        same = same && o.path[2 * i] == o.path[2 * (i + 350)] && o.path[2 * i + 1] == o.path[2 * (i + 350) + 1] && o.straight2[2 * i] == o.straight2[2 * (i + 350)];
        moved = moved || o.path[2 * i] != o.path[0];
    }
    CHECK(same && moved);
    ld_complex_destroy(c);
}

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: xlink_check <tests/golden> <scratch dir>\n");
        return 2;
    }
    tiny(argv[2]);
    czy(argv[1]);
    many(argv[2]);
    std::printf("xlink_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
