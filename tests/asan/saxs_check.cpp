// saxs_check.cpp -- driver of the sanitizer build of the small-angle scattering path (`make asan-saxs`;
// tests/test_asan_saxs.py): ld_complex_saxs_classes / ld_saxs_form_factors / ld_saxs_sinc / ld_complex_distance_histogram /
// ld_saxs_debye / ld_complex_saxs / ld_saxs_fit through the C ABI against tests/asan/hip_stub.cpp and
// tests/asan/hip_stub_saxs.cpp (device memory = host memory; the launches do the kernels' work in plain C++ from the shared
// rule, so the answers are real ones): the knife edges of a bin on two atoms, a file pair that hits all 21 pair classes
// against a count made here, the Debye sum against the ordered loop on the library's own tables, three 1czy poses in one
// chunk and in chunks of one, with and without zero-amplitude receptor modes, every NULL / non-NULL combination of the
// outputs, and every refusal by status with the outputs untouched.
//   usage: saxs_check <tests/golden> <scratch dir>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#define CHECK_PROGRAM "saxs_check"
#include "check.hpp"
#include "host/io.hpp"

static const uint32_t FILL = 0xA5A5A5A5u;
static const double DFILL = -7.25;

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

static std::vector<double> rigid(const std::vector<std::vector<double>> &t) {
    std::vector<double> poses(t.size() * 7, 0.0);
    for (size_t i = 0; i < t.size(); i++) {
        for (int k = 0; k < 3; k++) poses[i * 7 + k] = t[i][k];
        poses[i * 7 + 3] = 1.0;
    }
    return poses;
}

static bool all_fill(const std::vector<uint32_t> &v) {
    for (uint32_t x : v)
        if (x != FILL) return false;
    return true;
}
static bool all_fill(const std::vector<double> &v) {
    for (double x : v)
        if (x != DFILL) return false;
    return true;
}

static uint32_t pair_class(uint32_t e, uint32_t f) {
    const uint32_t lo = e < f ? e : f, hi = e < f ? f : e;
    return 6 * lo - lo * (lo - 1) / 2 + (hi - lo);
}

// The only non-zero word of a row of counts, or -1 when there is not exactly one pair.
static long only_word(const uint32_t *row, size_t words) {
    long at = -1;
    for (size_t i = 0; i < words; i++) {
        if (row[i] == 0) continue;
        if (row[i] != 1 || at >= 0) return -1;
        at = (long)i;
    }
    return at;
}

static void edges(const std::string &scratch) {
    ld_complex *c = two_files(scratch, "co", atom_line(1, "C", "GLY", 'A', 1, 0, 0, 0, rest("C").c_str()),
                              atom_line(1, "O", "HOH", 'B', 1, 0, 0, 0, rest("O").c_str()));
    CHECK(c != nullptr);
    if (!c) return;
    uint8_t cls[2] = {9, 9};
    CHECK(ld_complex_saxs_classes(c, 0, cls) == LD_OK && ld_complex_saxs_classes(c, 1, cls + 1) == LD_OK && cls[0] == 1 && cls[1] == 3);
    CHECK(ld_complex_saxs_classes(c, 2, cls) == LD_ERR_INVALID && ld_complex_saxs_classes(c, 0, nullptr) == LD_ERR_INVALID);
    CHECK(ld_complex_saxs_classes(nullptr, 0, cls) == LD_ERR_INVALID);
    const size_t bins = 8, words = 21 * bins, row = pair_class(1, 3) * bins;
    // printed distance k w -> bin k, k w - 1 -> bin k - 1; off the axis; the last bin
    const std::vector<std::vector<double>> t = {{0, 0, 0}, {0.499, 0, 0}, {0.5, 0, 0}, {1.499, 0, 0}, {1.5, 0, 0}, {0.3, 0.4, 0}, {0.299, 0.4, 0},
                                                {3.999, 0, 0}, {0, -3.5, 0}, {0, 0, -0.4994}, {0, 0, 0.4996}};
    const long want[] = {0, 0, 1, 2, 3, 1, 0, 7, 7, 0, 1};
    const std::vector<double> poses = rigid(t);
    std::vector<uint32_t> counts(t.size() * words, FILL);
    CHECK(ld_complex_distance_histogram(c, t.size(), poses.data(), 7, 500, bins, counts.data()) == LD_OK);
    for (size_t i = 0; i < t.size(); i++) CHECK(only_word(&counts[i * words], words) == (long)row + want[i]);
    // one bin beyond the last: refused, nothing written, whatever else the batch holds
    std::vector<double> beyond = rigid({{0.1, 0, 0}, {4.0, 0, 0}});
    std::vector<uint32_t> guard(2 * words, FILL);
    CHECK(ld_complex_distance_histogram(c, 2, beyond.data(), 7, 500, bins, guard.data()) == LD_ERR_INVALID && all_fill(guard));
    CHECK(ld_complex_distance_histogram(c, 2, beyond.data(), 7, 500, bins + 1, nullptr) == LD_OK);
    // the top of the range: 1023 x 2000 + 1999 along x and one thousandth off the axis
    const std::vector<double> top = rigid({{2047.999, 0.001, 0}, {2047.999, 0, 0}, {2048.0, 0, 0}, {2000.0, 443.4, 0}, {2000.0, 0.0, 441.0}});
    std::vector<uint32_t> wide(5 * 21 * 1024, FILL);
    CHECK(ld_complex_distance_histogram(c, 2, top.data(), 7, 2000, 1024, wide.data()) == LD_OK);
    CHECK(only_word(&wide[0], 21 * 1024) == (long)(pair_class(1, 3) * 1024 + 1023) && only_word(&wide[21 * 1024], 21 * 1024) == (long)(pair_class(1, 3) * 1024 + 1023));
    std::fill(wide.begin(), wide.end(), FILL);
    CHECK(ld_complex_distance_histogram(c, 3, top.data(), 7, 2000, 1024, wide.data()) == LD_ERR_INVALID && all_fill(wide));
    // off the axis beyond the last bin; a far pose is clamped and refused
    CHECK(ld_complex_distance_histogram(c, 1, top.data() + 3 * 7, 7, 2000, 1024, wide.data()) == LD_ERR_INVALID);
    CHECK(ld_complex_distance_histogram(c, 1, top.data() + 4 * 7, 7, 2000, 1024, wide.data()) == LD_ERR_INVALID && all_fill(wide));
    const std::vector<double> far = rigid({{9.0e5, -9.0e5, 5000.0}, {1.1e6, 0, 0}});
    CHECK(ld_complex_distance_histogram(c, 1, far.data(), 7, 2000, 1024, wide.data()) == LD_ERR_INVALID);
    CHECK(ld_complex_distance_histogram(c, 1, far.data() + 7, 7, 2000, 1024, wide.data()) == LD_ERR_INVALID && all_fill(wide));
    CHECK(ld_complex_distance_histogram(c, 0, nullptr, 7, 500, bins, nullptr) == LD_OK);

    // refusals: nothing written
    const double q[3] = {0.0, 0.1, 0.5};
    std::vector<double> I(t.size() * 3, DFILL);
    std::fill(counts.begin(), counts.end(), FILL);
    // hist: the histogram alone refuses it too (everything but q and n_q)
    auto refused = [&](const double *p, size_t stride, uint32_t width, size_t b, const double *qq, size_t n_q, bool hist = true) {
        const bool a = ld_complex_saxs(c, 2, p, stride, width, b, qq, n_q, I.data(), counts.data()) == LD_ERR_INVALID;
        const bool h = !hist || ld_complex_distance_histogram(c, 2, p, stride, width, b, counts.data()) == LD_ERR_INVALID;
        return a && h && all_fill(I) && all_fill(counts);
    };
    CHECK(refused(poses.data(), 7, 99, bins, q, 3) && refused(poses.data(), 7, 2001, bins, q, 3) && refused(poses.data(), 7, 0, bins, q, 3));
    CHECK(refused(poses.data(), 7, 500, 0, q, 3) && refused(poses.data(), 7, 500, 1025, q, 3));
    CHECK(refused(poses.data(), 7, 500, bins, q, 0, false) && refused(poses.data(), 7, 500, bins, nullptr, 3, false));
    {
        std::vector<double> many(1025, 0.1);
        CHECK(refused(poses.data(), 7, 500, bins, many.data(), 1025, false));
    }
    for (double bad : {-0.001, 1.001, (double)NAN, (double)INFINITY}) {
        const double qb[3] = {0.0, bad, 0.5};
        CHECK(refused(poses.data(), 7, 500, bins, qb, 3, false));
    }
    std::vector<double> bad = poses;
    bad[8] = NAN;
    CHECK(refused(bad.data(), 7, 500, bins, q, 3));
    bad = poses;
    bad[0] = INFINITY;
    CHECK(refused(bad.data(), 7, 500, bins, q, 3));
    bad = poses;
    bad[3] = 0.0;   // a zero quaternion
    CHECK(refused(bad.data(), 7, 500, bins, q, 3));
    CHECK(refused(poses.data(), 6, 500, bins, q, 3) && refused(nullptr, 7, 500, bins, q, 3));
    CHECK(ld_complex_saxs(nullptr, 2, poses.data(), 7, 500, bins, q, 3, I.data(), nullptr) == LD_ERR_INVALID && all_fill(I));

    // two atoms: I = f1^2 + f2^2 + 2 f1 f2 s(q r_k), on the library's own tables
    double f[3 * 6], s[3 * 8];
    CHECK(ld_saxs_form_factors(q, 3, f) == LD_OK && ld_saxs_sinc(q, 3, 500, bins, s) == LD_OK);
    CHECK(ld_complex_saxs(c, t.size(), poses.data(), 7, 500, bins, q, 3, I.data(), nullptr) == LD_OK);
    for (size_t i = 0; i < t.size(); i++)
        for (int j = 0; j < 3; j++) {
            const double f1 = f[j * 6 + 1], f2 = f[j * 6 + 3];
            CHECK(I[i * 3 + j] == (0.0 + 1.0 * (f1 * f1) + 1.0 * (f2 * f2)) + ((2.0 * f1) * f2) * (0.0 + 1.0 * s[j * 8 + want[i]]));
        }
    CHECK(s[0] == 1.0 && s[7] == 1.0 && s[8] == std::sin(0.1 * 0.25) / (0.1 * 0.25));
    ld_complex_destroy(c);

    // a complex of which no atom takes part
    c = two_files(scratch, "zn", atom_line(1, "ZN", "ZN", 'A', 1, 0, 0, 0, rest("ZN").c_str()), atom_line(1, "ZN", "ZN", 'B', 1, 0, 0, 0, rest("ZN").c_str()) + atom_line(2, "BJ", "MMB", 'B', 2, 1, 0, 0, rest("C").c_str()));
    CHECK(c != nullptr);
    if (!c) return;
    CHECK(ld_complex_saxs_classes(c, 1, cls) == LD_OK && cls[0] == 255 && cls[1] == 255);
    std::fill(I.begin(), I.end(), DFILL);
    CHECK(ld_complex_saxs(c, 2, poses.data(), 7, 500, bins, q, 3, I.data(), counts.data()) == LD_ERR_INVALID && all_fill(I) && all_fill(counts));
    CHECK(ld_complex_distance_histogram(c, 2, poses.data(), 7, 500, bins, counts.data()) == LD_ERR_INVALID && all_fill(counts));
    ld_complex_destroy(c);
}

struct Spot {
    const char *name, *res, *element;
    int x, y, z, cls;   // thousandths
};

// All six elements, a deuterium, a bead and a zinc over two files; every pair class is hit; the count is made here.
static void classes(const std::string &scratch) {
    const Spot rec[] = {{"H", "GLY", "H", 0, 0, 0, 0},       {"C", "GLY", "C", 1100, 0, 0, 1},     {"N", "GLY", "N", 0, 1300, 0, 2},  {"O", "GLY", "O", 0, 0, 1700, 3},
                        {"P", "DA", "P", 2300, 2300, 0, 4},  {"SG", "CYS", "S", 0, 2900, 2900, 5}, {"ZN", "ZN", "ZN", 500, 500, 500, 255},
                        {"BJ", "MMB", "C", 700, 700, 700, 255}};
    const Spot lig[] = {{"D1", "GLY", "D", 3100, 0, 0, 0},   {"CA", "GLY", "", 0, 3700, 0, 1},     {"N", "GLY", "N", 0, 0, 4100, 2},  {"O", "HOH", "O", 4300, 4300, 0, 3},
                        {"P", "DT", "P", 0, 4700, 4700, 4},  {"SD", "MET", "S", 5300, 0, 5300, 5}, {"1HB", "ALA", "", 5900, 5900, 5900, 0}};
    std::string rec_text, lig_text;
    std::vector<Spot> all;
    for (const Spot &a : rec) {
        all.push_back(a);
        rec_text += atom_line((int)all.size(), a.name, a.res, 'A', (int)all.size(), a.x / 1000.0, a.y / 1000.0, a.z / 1000.0, rest(a.element).c_str());
    }
    for (const Spot &a : lig) {
        all.push_back(a);
        lig_text += atom_line((int)all.size(), a.name, a.res, 'B', (int)all.size(), a.x / 1000.0, a.y / 1000.0, a.z / 1000.0, rest(a.element).c_str());
    }
    ld_complex *c = two_files(scratch, "six", rec_text, lig_text);
    CHECK(c != nullptr);
    if (!c) return;
    uint8_t cls[15];
    CHECK(ld_complex_saxs_classes(c, 0, cls) == LD_OK && ld_complex_saxs_classes(c, 1, cls + 8) == LD_OK);
    for (size_t a = 0; a < all.size(); a++) CHECK(cls[a] == all[a].cls);
    const int shift[2][3] = {{0, 0, 0}, {-1234, 777, 2001}};
    const std::vector<double> poses = rigid({{0, 0, 0}, {-1.234, 0.777, 2.001}});
    const size_t bins = 40, words = 21 * bins;
    const uint32_t w = 400;
    std::vector<uint32_t> counts(2 * words, FILL), want(2 * words, 0);
    CHECK(ld_complex_distance_histogram(c, 2, poses.data(), 7, w, bins, counts.data()) == LD_OK);
    for (int i = 0; i < 2; i++)
        for (size_t a = 0; a < all.size(); a++)
            for (size_t b = a + 1; b < all.size(); b++) {
                if (all[a].cls == 255 || all[b].cls == 255) continue;
                const long long sa = a >= 8, sb = b >= 8;
                const long long dx = all[a].x + sa * shift[i][0] - all[b].x - sb * shift[i][0], dy = all[a].y + sa * shift[i][1] - all[b].y - sb * shift[i][1],
                                dz = all[a].z + sa * shift[i][2] - all[b].z - sb * shift[i][2];
                const long long d2 = dx * dx + dy * dy + dz * dz;
                long long k = 0;
                while ((k + 1) * w * (k + 1) * w <= d2) k++;
                want[i * words + pair_class((uint32_t)all[a].cls, (uint32_t)all[b].cls) * bins + (size_t)k]++;
            }
    CHECK(counts == want);
    for (int cl = 0; cl < 21; cl++) {
        uint32_t total = 0;
        for (size_t k = 0; k < bins; k++) total += counts[cl * bins + k];
        CHECK(total > 0);
    }

    // the Debye sum, alone and in one call with the histogram, against the ordered loop on the library's own tables
    const double q[4] = {0.0, 0.05, 0.3, 1.0};
    const uint32_t n_e[6] = {3, 2, 2, 2, 2, 2};
    std::vector<double> f(4 * 6), s(4 * bins), I(2 * 4, DFILL), J(2 * 4, DFILL), expect(2 * 4);
    CHECK(ld_saxs_form_factors(q, 4, f.data()) == LD_OK && ld_saxs_sinc(q, 4, w, bins, s.data()) == LD_OK);
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 4; j++) {
            double S = 0.0;
            for (int e = 0; e < 6; e++) S = S + (double)n_e[e] * (f[j * 6 + e] * f[j * 6 + e]);
            double sum = S;
            for (int e = 0; e < 6; e++)
                for (int g = e; g < 6; g++) {
                    double G = 0.0;
                    for (size_t k = 0; k < bins; k++) G = G + (double)counts[i * words + pair_class(e, g) * bins + k] * s[j * bins + k];
                    sum = sum + ((2.0 * f[j * 6 + e]) * f[j * 6 + g]) * G;
                }
            expect[i * 4 + j] = sum;
        }
    CHECK(ld_saxs_debye(2, counts.data(), w, bins, n_e, q, 4, I.data()) == LD_OK && I == expect);
    for (int mask = 0; mask < 4; mask++) {
        std::vector<uint32_t> again(2 * words, FILL);
        std::fill(J.begin(), J.end(), DFILL);
        CHECK(ld_complex_saxs(c, 2, poses.data(), 7, w, bins, q, 4, mask & 1 ? J.data() : nullptr, mask & 2 ? again.data() : nullptr) == LD_OK);
        CHECK(mask & 1 ? J == expect : all_fill(J));
        CHECK(mask & 2 ? again == counts : all_fill(again));
    }
    // synthetic counts: zero rows, a single full bin, values near 2^32
    std::vector<uint32_t> synth(3 * words, 0);
    synth[words + 7 * bins + 11] = 0xFFFFFFFFu;
    for (size_t i = 0; i < words; i++) synth[2 * words + i] = 0xFFFFFF00u + (uint32_t)(i % 255);
    std::vector<double> K(3 * 4, DFILL);
    CHECK(ld_saxs_debye(3, synth.data(), w, bins, n_e, q, 4, K.data()) == LD_OK);
    for (int j = 0; j < 4; j++) {
        double S = 0.0;
        for (int e = 0; e < 6; e++) S = S + (double)n_e[e] * (f[j * 6 + e] * f[j * 6 + e]);
        CHECK(K[j] == S);
        CHECK(K[4 + j] == S + ((2.0 * f[j * 6 + 1]) * f[j * 6 + 2]) * (0.0 + 4294967295.0 * s[j * bins + 11]));   // pair class 7 is (C, N)
    }
    CHECK(std::isfinite(K[8]) && K[8] != K[0]);
    // ld_saxs_debye's refusals
    std::fill(K.begin(), K.end(), DFILL);
    CHECK(ld_saxs_debye(3, synth.data(), 99, bins, n_e, q, 4, K.data()) == LD_ERR_INVALID && ld_saxs_debye(3, synth.data(), w, 0, n_e, q, 4, K.data()) == LD_ERR_INVALID);
    CHECK(ld_saxs_debye(3, synth.data(), w, bins, n_e, q, 0, K.data()) == LD_ERR_INVALID && ld_saxs_debye(3, synth.data(), w, bins, nullptr, q, 4, K.data()) == LD_ERR_INVALID);
    CHECK(ld_saxs_debye(3, nullptr, w, bins, n_e, q, 4, K.data()) == LD_ERR_INVALID && ld_saxs_debye(3, synth.data(), w, bins, n_e, q, 4, nullptr) == LD_ERR_INVALID);
    CHECK(all_fill(K) && ld_saxs_debye(0, nullptr, w, bins, n_e, q, 4, nullptr) == LD_OK);

    // the fit
    const double i_exp[4] = {2.0 * expect[0], 2.0 * expect[1], 2.0 * expect[2], 2.0 * expect[3]}, sigma[4] = {1.0, 2.0, 0.5, 0.1};
    double scale[2] = {DFILL, DFILL}, chi2[2] = {DFILL, DFILL};
    CHECK(ld_saxs_fit(2, 4, expect.data(), i_exp, sigma, scale, chi2) == LD_OK && scale[0] == 2.0 && chi2[0] == 0.0 && chi2[1] > 0.0);
    for (int mask = 0; mask < 4; mask++) {
        double sc[2] = {DFILL, DFILL}, ch[2] = {DFILL, DFILL};
        CHECK(ld_saxs_fit(2, 4, expect.data(), i_exp, sigma, mask & 1 ? sc : nullptr, mask & 2 ? ch : nullptr) == LD_OK);
        CHECK((mask & 1 ? sc[1] == scale[1] : sc[1] == DFILL) && (mask & 2 ? ch[1] == chi2[1] : ch[1] == DFILL));
    }
    const double bad_sigma[4] = {1.0, 0.0, 0.5, 0.1}, zeros[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double sc[2] = {DFILL, DFILL}, ch[2] = {DFILL, DFILL};
    CHECK(ld_saxs_fit(2, 4, expect.data(), i_exp, bad_sigma, sc, ch) == LD_ERR_INVALID && ld_saxs_fit(2, 4, zeros, i_exp, sigma, sc, ch) == LD_ERR_INVALID);
    CHECK(ld_saxs_fit(2, 0, expect.data(), i_exp, sigma, sc, ch) == LD_ERR_INVALID && ld_saxs_fit(2, 4, nullptr, i_exp, sigma, sc, ch) == LD_ERR_INVALID);
    CHECK(sc[0] == DFILL && sc[1] == DFILL && ch[0] == DFILL && ch[1] == DFILL && ld_saxs_fit(0, 4, nullptr, i_exp, sigma, sc, ch) == LD_OK);
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
    const size_t len = ld_complex_pose_len(c), n_rec = ld_complex_num_atoms(c, 0), atoms = n_rec + ld_complex_num_atoms(c, 1);
    CHECK(len == 27);
    std::vector<uint8_t> cls(atoms);
    CHECK(ld_complex_saxs_classes(c, 0, cls.data()) == LD_OK && ld_complex_saxs_classes(c, 1, cls.data() + n_rec) == LD_OK);
    uint64_t part = 0;
    for (uint8_t e : cls) part += e != 255;
    CHECK(part > 1000 && part <= atoms);
    const size_t stride = len + 2, n = 3, bins = 300, words = 21 * bins;
    std::vector<double> poses(n * stride, 0.0);
    const std::vector<double> first = gso_pose(d + "swarm_2/gso_100.out", 74), second = gso_pose(d + "swarm_0/gso_100.out", 0),
                              third = gso_pose(d + "swarm_9/gso_100.out", 199);
    CHECK(first.size() == 27 && second.size() == 27 && third.size() == 27);
    if (first.size() != 27 || second.size() != 27 || third.size() != 27) return;
    std::copy(first.begin(), first.end(), poses.begin());
    std::copy(second.begin(), second.end(), poses.begin() + stride);
    std::copy(third.begin(), third.end(), poses.begin() + 2 * stride);
    std::vector<uint32_t> counts(n * words, FILL), pieces(n * words, FILL);
    CHECK(ld_complex_distance_histogram(c, n, poses.data(), stride, 500, bins, counts.data()) == LD_OK);
    for (size_t i = 0; i < n; i++) {
        uint64_t total = 0;
        for (size_t k = 0; k < words; k++) total += counts[i * words + k];
        CHECK(total == part * (part - 1) / 2);
    }
    CHECK(std::memcmp(&counts[0], &counts[words], words * sizeof(uint32_t)) != 0);
    double ms = -1.0;
    CHECK(ld_complex_last_kernel_ms(c, &ms) == LD_OK && ms == 0.0);
    // chunks of one pose; the poses in another order
    CHECK(ld_complex_saxs_chunk(c, 1) == LD_OK && ld_complex_saxs_chunk(nullptr, 1) == LD_ERR_INVALID);
    CHECK(ld_complex_distance_histogram(c, n, poses.data(), stride, 500, bins, pieces.data()) == LD_OK && pieces == counts);
    const double q[2] = {0.02, 0.4};
    std::vector<double> I(n * 2, DFILL), J(n * 2, DFILL);
    CHECK(ld_complex_saxs(c, n, poses.data(), stride, 500, bins, q, 2, I.data(), nullptr) == LD_OK);
    CHECK(ld_complex_saxs_chunk(c, 0) == LD_OK);
    CHECK(ld_complex_saxs(c, n, poses.data(), stride, 500, bins, q, 2, J.data(), pieces.data()) == LD_OK && I == J && pieces == counts);
    std::vector<uint32_t> one(words, FILL);
    CHECK(ld_complex_distance_histogram(c, 1, poses.data() + 2 * stride, stride, 500, bins, one.data()) == LD_OK);
    CHECK(std::memcmp(one.data(), &counts[2 * words], words * sizeof(uint32_t)) == 0);
    // too few bins for 1czy: refused, nothing written
    std::fill(pieces.begin(), pieces.end(), FILL);
    CHECK(ld_complex_distance_histogram(c, n, poses.data(), stride, 500, 40, pieces.data()) == LD_ERR_INVALID && all_fill(pieces));
    ld_complex_destroy(c);

    // a receptor without modes: the base row; the same complex with zero-amplitude receptor modes: no base row
    std::vector<double> rigid_rec(n * 17, 0.0), flexible(n * 27, 0.0);
    for (size_t i = 0; i < n; i++) {
        std::copy(&poses[i * stride], &poses[i * stride] + 7, &rigid_rec[i * 17]);
        std::copy(&poses[i * stride] + 17, &poses[i * stride] + 27, &rigid_rec[i * 17 + 7]);
        std::copy(&poses[i * stride], &poses[i * stride] + 7, &flexible[i * 27]);
        std::copy(&poses[i * stride] + 17, &poses[i * stride] + 27, &flexible[i * 27 + 17]);
    }
    ld_complex *a = ld_complex_create(rec.c_str(), lig.c_str(), nullptr, 0, 0, lig_nm.data(), lig_nm.size(), 10);
    ld_complex *b = ld_complex_create(rec.c_str(), lig.c_str(), rec_nm.data(), rec_nm.size(), 10, lig_nm.data(), lig_nm.size(), 10);
    CHECK(a != nullptr && b != nullptr);
    if (a && b) {
        std::vector<uint32_t> ca(n * words, FILL), cb(n * words, FILL);
        CHECK(ld_complex_distance_histogram(a, n, rigid_rec.data(), 17, 500, bins, ca.data()) == LD_OK);
        CHECK(ld_complex_distance_histogram(b, n, flexible.data(), 27, 500, bins, cb.data()) == LD_OK && ca == cb);
        CHECK(ca != counts);
    }
    ld_complex_destroy(a);
    ld_complex_destroy(b);
}

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: saxs_check <tests/golden> <scratch dir>\n");
        return 2;
    }
    edges(argv[2]);
    classes(argv[2]);
    czy(argv[1]);
    std::printf("saxs_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
