// sasa_check.cpp -- driver of the sanitizer build of the solvent-accessible surface path (`make asan-sasa`;
// tests/test_asan_sasa.py): ld_sasa_directions / ld_complex_sasa_radii / ld_complex_sasa through the C ABI against
// tests/asan/hip_stub.cpp and tests/asan/hip_stub_sasa.cpp (device memory = host memory; the launch does the kernel's work
// in plain C++ from the shared rule, so the answers are real ones): tiny cases whose counts the rule's text pins, a few
// 1czy poses (the first ranked model's sums are pinned too), more poses than workspace slots, every NULL / non-NULL
// combination of the outputs, and every refusal by status with the outputs untouched.
//   usage: sasa_check <tests/golden> <scratch dir>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#define CHECK_PROGRAM "sasa_check"
#include "check.hpp"
#include "host/io.hpp"

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
    std::vector<uint64_t> sums;
    std::vector<uint8_t> free_counts, bound_counts;
    Out(size_t n, size_t atoms) : sums(n * 4, 0xA5A5A5A5A5A5A5A5ull), free_counts(n * atoms, 0xA5), bound_counts(n * atoms, 0xA5) {}
    bool untouched() const {
        for (uint64_t v : sums)
            if (v != 0xA5A5A5A5A5A5A5A5ull) return false;
        for (uint8_t v : free_counts)
            if (v != 0xA5) return false;
        for (uint8_t v : bound_counts)
            if (v != 0xA5) return false;
        return true;
    }
};

static std::vector<double> rigid(size_t n, const std::vector<double> &tx) {
    std::vector<double> poses(n * 7, 0.0);
    for (size_t i = 0; i < n; i++) poses[i * 7] = tx[i], poses[i * 7 + 3] = 1.0;
    return poses;
}

static void tiny(const std::string &scratch) {
    int32_t U[LD_SASA_POINTS * 3];
    CHECK(ld_sasa_directions(U) == LD_OK && ld_sasa_directions(nullptr) == LD_ERR_INVALID);
    CHECK(U[0] == 130816 && U[1] == 0 && U[2] == 1040384 && U[3] == -166416 && U[3 * 64] == -988382 && U[3 * 127 + 2] == -1040384);

    // two carbons, one a molecule; a hydrogen and a bead between them cover nothing
    ld_complex *c = two_files(scratch, "cc", atom_line(1, "C", "GLY", 'A', 1, 0, 0, 0, rest("C").c_str()) + atom_line(2, "H", "GLY", 'A', 1, 1.5, 0, 0, rest("H").c_str()),
                              atom_line(1, "BJ", "MMB", 'B', 1, -1.5, 0, 0, rest("C").c_str()) + atom_line(2, "C", "GLY", 'B', 2, 0, 0, 0, rest("C").c_str()));
    CHECK(c != nullptr);
    if (!c) return;
    uint32_t radii[4] = {7, 7, 7, 7};
    CHECK(ld_complex_sasa_radii(c, 0, radii) == LD_OK && radii[0] == 1700 && radii[1] == 0);
    CHECK(ld_complex_sasa_radii(c, 1, radii + 2) == LD_OK && radii[2] == 0 && radii[3] == 1700);
    CHECK(ld_complex_sasa_radii(c, 2, radii) == LD_ERR_INVALID && ld_complex_sasa_radii(c, 0, nullptr) == LD_ERR_INVALID);
    CHECK(ld_complex_sasa_radii(nullptr, 0, radii) == LD_ERR_INVALID);
    const std::vector<double> tx = {0.0, 0.001, 3.0, 3.0034, 3.004, 6.2, 500.0, -0.9e6};
    const std::vector<double> poses = rigid(tx.size(), tx);
    Out o(tx.size(), 4);
    CHECK(ld_complex_sasa(c, tx.size(), poses.data(), 7, 1.4, o.sums.data(), o.free_counts.data(), o.bound_counts.data()) == LD_OK);
    const int want[8][2] = {{69, 69}, {66, 64}, {95, 95}, {95, 95}, {95, 96}, {128, 128}, {128, 128}, {128, 128}};
    for (size_t i = 0; i < tx.size(); i++) {
        const uint8_t *f = &o.free_counts[i * 4], *b = &o.bound_counts[i * 4];
        CHECK(f[0] == 128 && f[1] == 0 && f[2] == 0 && f[3] == 128);
        CHECK(b[0] == want[i][0] && b[1] == 0 && b[2] == 0 && b[3] == want[i][1]);
        const uint64_t E2 = 3100ull * 3100ull;
        CHECK(o.sums[4 * i] == 128 * E2 && o.sums[4 * i + 1] == (uint64_t)want[i][0] * E2 && o.sums[4 * i + 2] == 128 * E2 &&
              o.sums[4 * i + 3] == (uint64_t)want[i][1] * E2);
    }
    // a probe of 0: the spheres of two carbons 3.41 A apart do not meet and bury nothing; at 2.0 A they do
    const std::vector<double> apart = rigid(1, {3.41});
    Out z(1, 4);
    CHECK(ld_complex_sasa(c, 1, apart.data(), 7, 0.0, z.sums.data(), nullptr, z.bound_counts.data()) == LD_OK);
    CHECK(z.bound_counts[0] == 128 && z.bound_counts[3] == 128 && z.sums[1] == 128ull * 1700 * 1700);
    CHECK(ld_complex_sasa(c, 1, apart.data(), 7, 2.0, z.sums.data(), nullptr, nullptr) == LD_OK && z.sums[1] < z.sums[0] && z.sums[0] == 128ull * 3700 * 3700);
    ld_complex_destroy(c);

    // C against O; radii by element column, by atom name, of a 54-column record
    c = two_files(scratch, "co", atom_line(1, "C", "GLY", 'A', 1, 0, 0, 0, rest("C").c_str()),
                  atom_line(1, "O", "HOH", 'B', 1, 0, 0, 0, rest("O").c_str()) + atom_line(2, "ZN", "ZN", 'B', 2, 50, 0, 0, rest("ZN").c_str()) +
                      atom_line(3, "CA", "GLY", 'B', 3, 60, 0, 0, rest("").c_str()) + atom_line(4, "N", "GLY", 'B', 3, 70, 0, 0) + "\n" +
                      atom_line(5, "1HB", "ALA", 'B', 4, 80, 0, 0, rest("").c_str()) + atom_line(6, "SE", "MSE", 'B', 5, 90, 0, 0, rest("se").c_str()));
    CHECK(c != nullptr);
    if (!c) return;
    uint32_t r6[6];
    CHECK(ld_complex_sasa_radii(c, 1, r6) == LD_OK && r6[0] == 1520 && r6[1] == 1800 && r6[2] == 1700 && r6[3] == 1550 && r6[4] == 0 && r6[5] == 1900);
    const std::vector<double> three = rigid(1, {3.0});
    Out co(1, 7);
    CHECK(ld_complex_sasa(c, 1, three.data(), 7, 1.4, co.sums.data(), co.free_counts.data(), co.bound_counts.data()) == LD_OK);
    CHECK(co.bound_counts[0] == 99 && co.bound_counts[1] == 92 && co.free_counts[5] == 0 && co.free_counts[6] == 128);
    ld_complex_destroy(c);

    // a side of which no atom takes part: refused, nothing written
    c = two_files(scratch, "hh", atom_line(1, "C", "GLY", 'A', 1, 0, 0, 0, rest("C").c_str()),
                  atom_line(1, "H", "GLY", 'B', 1, 0, 0, 0, rest("H").c_str()) + atom_line(2, "BJ", "MMB", 'B', 2, 1, 0, 0, rest("C").c_str()));
    CHECK(c != nullptr);
    if (!c) return;
    Out h(1, 3);
    CHECK(ld_complex_sasa(c, 1, three.data(), 7, 1.4, h.sums.data(), h.free_counts.data(), h.bound_counts.data()) == LD_ERR_INVALID && h.untouched());
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
    ld_complex *c = ld_complex_create((d + "lightdock_1czy_protein.pdb").c_str(), (d + "lightdock_1czy_peptide.pdb").c_str(), rec_nm.data(),
                                      rec_nm.size(), 10, lig_nm.data(), lig_nm.size(), 10);
    CHECK(c != nullptr);
    if (!c) return;
    const size_t len = ld_complex_pose_len(c), atoms = ld_complex_num_atoms(c, 0) + ld_complex_num_atoms(c, 1), n_rec = ld_complex_num_atoms(c, 0);
    CHECK(len == 27);
    std::vector<uint32_t> radii(atoms);
    CHECK(ld_complex_sasa_radii(c, 0, radii.data()) == LD_OK && ld_complex_sasa_radii(c, 1, radii.data() + n_rec) == LD_OK);
    const size_t stride = len + 2, n = 3;
    std::vector<double> poses(n * stride, 0.0);
    const std::vector<double> first = gso_pose(d + "swarm_2/gso_100.out", 74), second = gso_pose(d + "swarm_0/gso_100.out", 0),
                              third = gso_pose(d + "swarm_9/gso_100.out", 199);
    CHECK(first.size() == 27 && second.size() == 27 && third.size() == 27);
    if (first.size() != 27 || second.size() != 27 || third.size() != 27) return;
    std::copy(first.begin(), first.end(), poses.begin());
    std::copy(second.begin(), second.end(), poses.begin() + stride);
    std::copy(third.begin(), third.end(), poses.begin() + 2 * stride);
    Out o(n, atoms);
    CHECK(ld_complex_sasa(c, n, poses.data(), stride, 1.4, o.sums.data(), o.free_counts.data(), o.bound_counts.data()) == LD_OK);
    CHECK(o.sums[0] == 87964903100ull && o.sums[1] == 83835702000ull && o.sums[2] == 10636044500ull && o.sums[3] == 5434214900ull);
    for (size_t i = 0; i < n; i++) {   // the sums are those of the counts; bound <= free <= 128; nothing for an atom that takes no part
        uint64_t s[4] = {0, 0, 0, 0};
        bool ordered = true;
        for (size_t a = 0; a < atoms; a++) {
            const uint64_t E = radii[a] ? radii[a] + 1400 : 0, f = o.free_counts[i * atoms + a], b = o.bound_counts[i * atoms + a];
            ordered = ordered && b <= f && f <= 128 && (radii[a] || f == 0);
            s[a < n_rec ? 0 : 2] += f * E * E;
            s[a < n_rec ? 1 : 3] += b * E * E;
        }
        CHECK(ordered && s[0] == o.sums[4 * i] && s[1] == o.sums[4 * i + 1] && s[2] == o.sums[4 * i + 2] && s[3] == o.sums[4 * i + 3]);
        CHECK(o.sums[4 * i + 1] < o.sums[4 * i] && o.sums[4 * i + 3] < o.sums[4 * i + 2]);
    }
    // every NULL / non-NULL combination gives the same numbers
    for (int mask = 0; mask < 8; mask++) {
        Out p(n, atoms);
        CHECK(ld_complex_sasa(c, n, poses.data(), stride, 1.4, mask & 1 ? p.sums.data() : nullptr, mask & 2 ? p.free_counts.data() : nullptr,
                              mask & 4 ? p.bound_counts.data() : nullptr) == LD_OK);
        CHECK(!(mask & 1) || p.sums == o.sums);
        CHECK(!(mask & 2) || p.free_counts == o.free_counts);
        CHECK(!(mask & 4) || p.bound_counts == o.bound_counts);
        if (mask == 0) CHECK(p.untouched());
    }
    CHECK(ld_complex_sasa(c, 0, nullptr, len, 1.4, nullptr, nullptr, nullptr) == LD_OK);
    double ms = -1.0;
    CHECK(ld_complex_last_kernel_ms(c, &ms) == LD_OK && ms == 0.0);

    // refusals: nothing written
    Out r(n, atoms);
    auto refused = [&](const double *p, size_t st, double probe) {
        return ld_complex_sasa(c, n, p, st, probe, r.sums.data(), r.free_counts.data(), r.bound_counts.data()) == LD_ERR_INVALID && r.untouched();
    };
    for (double probe : {-0.001, -1.0, 2.001, (double)NAN, (double)INFINITY, -(double)INFINITY, 1e300}) CHECK(refused(poses.data(), stride, probe));
    std::vector<double> bad = poses;
    bad[stride + 5] = NAN;
    CHECK(refused(bad.data(), stride, 1.4));
    bad = poses;
    bad[2 * stride + 1] = INFINITY;
    CHECK(refused(bad.data(), stride, 1.4));
    bad = poses;
    for (int k = 3; k < 7; k++) bad[stride + k] = 0.0;   // a zero quaternion
    CHECK(refused(bad.data(), stride, 1.4));
    CHECK(refused(poses.data(), len - 1, 1.4) && refused(nullptr, stride, 1.4));
    bad = poses;
    bad[2 * stride] = 1.1e6;   // beyond the coordinate bound: found by the launch, after it wrote device memory
    CHECK(refused(bad.data(), stride, 1.4));
    bad[2 * stride] = -0.9e6;  // inside it
    CHECK(ld_complex_sasa(c, n, bad.data(), stride, 1.4, r.sums.data(), nullptr, nullptr) == LD_OK && r.sums[8] == r.sums[9] && r.sums[10] == r.sums[11]);
    CHECK(ld_complex_sasa(nullptr, n, poses.data(), stride, 1.4, r.sums.data(), nullptr, nullptr) == LD_ERR_INVALID);
    ld_complex_destroy(c);
}

// More poses than workspace slots, on a complex small enough for the stub's all-pairs walk.
static void many(const std::string &scratch) {
    ld_complex *c = two_files(scratch, "many", atom_line(1, "N", "GLY", 'A', 1, 0, 0, 0, rest("N").c_str()) + atom_line(2, "CA", "GLY", 'A', 1, 1.5, 0, 0, rest("C").c_str()),
                              atom_line(1, "P", "DT", 'B', 1, 0, 0, 0, rest("P").c_str()));
    CHECK(c != nullptr);
    if (!c) return;
    const size_t n = 2500;
    std::vector<double> tx(n);
    for (size_t i = 0; i < n; i++) tx[i] = 0.004 * (double)i;
    const std::vector<double> poses = rigid(n, tx);
    Out o(n, 3);
    CHECK(ld_complex_sasa(c, n, poses.data(), 7, 1.4, o.sums.data(), o.free_counts.data(), o.bound_counts.data()) == LD_OK);
    CHECK(o.free_counts[0] == o.free_counts[3 * (n - 1)] && o.free_counts[2] == 128 && o.bound_counts[3 * (n - 1) + 2] == 128);
    CHECK(o.bound_counts[2] < 128 && o.sums[4 * (n - 1) + 2] == 128ull * 3200 * 3200);
    ld_complex_destroy(c);
}

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: sasa_check <tests/golden> <scratch dir>\n");
        return 2;
    }
    tiny(argv[2]);
    czy(argv[1]);
    many(argv[2]);
    std::printf("sasa_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
