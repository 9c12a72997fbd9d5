// emfit_check.cpp -- driver of the sanitizer build of the density-fit path (`make asan-emfit`; tests/test_asan_emfit.py):
// ld_density_create / _info / _voxels / _kernel / _scores, ld_complex_density_fit / _simulate_density / _density_chunk through
// the C ABI against tests/asan/hip_stub.cpp and tests/asan/hip_stub_emfit.cpp (device memory = host memory; the launches do
// the kernels' work in plain C++ from the shared rule, so the answers are real ones): the quantisation and its refusals, the
// table's plan, a two-atom complex on a 2 x 1 x 1 map worked out by hand, clipping and `outside`, three 1czy poses in one
// chunk and in chunks of one, with a rigid receptor and with zero-amplitude receptor modes, the sums against the voxels, the
// scores' degenerate cases, and every refusal by status with the outputs untouched.
//   usage: emfit_check <tests/golden> <scratch dir>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#define CHECK_PROGRAM "emfit_check"
#include "check.hpp"
#include "host/io.hpp"

static const uint32_t FILL = 0xA5A5A5A5u;

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

static bool sums_filled(const std::vector<ld_density_sums> &v) {
    const unsigned char *p = reinterpret_cast<const unsigned char *>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(ld_density_sums); i++)
        if (p[i] != 0xA5) return false;
    return true;
}

static std::vector<ld_density_sums> filled(size_t n) {
    std::vector<ld_density_sums> v(n);
    std::memset(v.data(), 0xA5, n * sizeof(ld_density_sums));
    return v;
}

static bool same(const ld_density_sums &a, const ld_density_sums &b) {
    return a.s == b.s && a.ss == b.ss && a.se == b.se && a.inside_sum == b.inside_sum && a.outside == b.outside;
}

static void maps_and_tables() {
    const uint32_t n[3] = {2, 2, 1}, step[3] = {1000, 1000, 1000};
    const int32_t origin[3] = {0, 0, 0};
    const float rho[4] = {-1.0f, 0.5f, 2.0f, 1.0f};
    ld_density *d = ld_density_create(rho, n, origin, step, 0.0);
    CHECK(d != nullptr);
    if (d) {
        uint64_t N = 0, se = 0, see = 0;
        double scale = 0.0;
        uint32_t E[4] = {FILL, FILL, FILL, FILL};
        CHECK(ld_density_info(d, &N, &se, &see, &scale) == LD_OK && N == 4 && scale == 32767.0 / 2.0);
        CHECK(ld_density_voxels(d, E) == LD_OK && E[0] == 0 && E[1] == 8192 && E[2] == 32767 && E[3] == 16384);   // 8191.75, 16383.5 -> even
        CHECK(se == 8192 + 32767 + 16384 && see == 8192ull * 8192 + 32767ull * 32767 + 16384ull * 16384);
        CHECK(ld_density_info(d, nullptr, nullptr, nullptr, nullptr) == LD_OK && ld_density_voxels(d, nullptr) == LD_ERR_INVALID);
        ld_density_destroy(d);
    }
    d = ld_density_create(rho, n, origin, step, 0.75);   // 0.5 falls below the threshold
    CHECK(d != nullptr);
    if (d) {
        uint32_t E[4];
        CHECK(ld_density_voxels(d, E) == LD_OK && E[0] == 0 && E[1] == 0 && E[2] == 32767 && E[3] == 16384);
        ld_density_destroy(d);
    }
    const float nan_rho[4] = {1.0f, NAN, 1.0f, 1.0f}, none[4] = {0.0f, -1.0f, 0.0f, 0.0f};
    const uint32_t zero_n[3] = {0, 2, 1}, big_n[3] = {1025, 1, 1}, small_step[3] = {199, 1000, 1000}, big_step[3] = {1000, 20001, 1000};
    const int32_t far[3] = {0, 1000000001, 0};
    CHECK(ld_density_create(nan_rho, n, origin, step, 0.0) == nullptr && ld_density_create(none, n, origin, step, 0.0) == nullptr);
    CHECK(ld_density_create(rho, n, origin, step, 2.5) == nullptr && ld_density_create(rho, n, origin, step, -1.0) == nullptr);
    CHECK(ld_density_create(rho, zero_n, origin, step, 0.0) == nullptr && ld_density_create(rho, big_n, origin, step, 0.0) == nullptr);
    CHECK(ld_density_create(rho, n, origin, small_step, 0.0) == nullptr && ld_density_create(rho, n, origin, big_step, 0.0) == nullptr);
    CHECK(ld_density_create(rho, n, far, step, 0.0) == nullptr && ld_density_create(nullptr, n, origin, step, 0.0) == nullptr);
    ld_density_destroy(nullptr);

    // the table: length, shift, the first and last entries
    uint32_t length = 0, shift = 99;
    CHECK(ld_density_kernel(300, nullptr, &length, &shift) == LD_OK && shift == 9 && length > 2048 && length <= 4096);
    std::vector<uint32_t> K(length + 1, FILL);
    CHECK(ld_density_kernel(300, K.data(), &length, &shift) == LD_OK && K[0] == 255 && K[length - 1] <= 1 && K[length] == FILL);
    for (uint32_t t = 1; t < length; t++) CHECK(K[t] <= K[t - 1]);
    CHECK(ld_density_kernel(15000, nullptr, &length, &shift) == LD_OK && shift == 20 && length == 2676);
    CHECK(ld_density_kernel(299, nullptr, &length, &shift) == LD_ERR_INVALID && ld_density_kernel(15001, nullptr, &length, &shift) == LD_ERR_INVALID);
    CHECK(ld_density_kernel(300, nullptr, nullptr, nullptr) == LD_OK);
}

static void by_hand(const std::string &scratch) {
    // a carbon at the origin (receptor) and an oxygen 1 A along x (ligand) on two voxels at x = 0 and x = 1 A
    ld_complex *c = two_files(scratch, "em", atom_line(1, "C", "GLY", 'A', 1, 0, 0, 0, rest("C").c_str()),
                              atom_line(1, "O", "HOH", 'B', 1, 0, 0, 0, rest("O").c_str()));
    CHECK(c != nullptr);
    if (!c) return;
    const uint32_t n[3] = {2, 1, 1}, step[3] = {1000, 1000, 1000};
    const int32_t origin[3] = {0, 0, 0};
    const float rho[2] = {1.0f, 0.0f};
    ld_density *d = ld_density_create(rho, n, origin, step, 0.0);
    CHECK(d != nullptr);
    if (!d) return;
    uint32_t length = 0, shift = 0;
    CHECK(ld_density_kernel(300, nullptr, &length, &shift) == LD_OK);
    std::vector<uint32_t> K(length);
    CHECK(ld_density_kernel(300, K.data(), &length, &shift) == LD_OK);
    const uint32_t k0 = K[0], k1 = K[1000000u >> shift];   // d^2 = 0 and d^2 = 10^6
    const double poses[3 * 7] = {1.0, 0, 0, 1, 0, 0, 0, /* outside the grid's cells */ 1.5, 0, 0, 1, 0, 0, 0, /* far away */ 500.0, 0, 0, 1, 0, 0, 0};
    std::vector<uint32_t> grid(3 * 2, FILL);
    CHECK(ld_complex_simulate_density(c, d, 3, poses, 7, 300, grid.data()) == LD_OK);
    CHECK(grid[0] == 6 * k0 + 8 * k1 && grid[1] == 6 * k1 + 8 * k0);
    CHECK(grid[4] == 6 * k0 && grid[5] == 6 * k1);
    std::vector<ld_density_sums> sums = filled(3);
    CHECK(ld_complex_density_fit(c, d, 3, poses, 7, 300, sums.data()) == LD_OK);
    const uint64_t a = grid[0], b = grid[1];
    CHECK(sums[0].s == a + b && sums[0].ss == a * a + b * b && sums[0].se == a * 32767 && sums[0].inside_sum == a && sums[0].outside == 0 && sums[0].reserved == 0);
    CHECK(sums[1].outside == 1 && sums[2].outside == 1 && sums[2].s == 6ull * (k0 + k1));
    double cc[3], ccm[3], inside[3];
    CHECK(ld_density_scores(d, 3, sums.data(), cc, ccm, inside) == LD_OK);
    CHECK(cc[0] == (double)(a * 32767) / (std::sqrt((double)(a * a + b * b)) * std::sqrt((double)(32767ull * 32767))));
    CHECK(inside[0] == (double)a / (double)(a + b) && a < b && ccm[0] == -1.0);   // two voxels, the oxygen on the empty one
    for (int mask = 0; mask < 8; mask++) {
        double x[3] = {-7.0, -7.0, -7.0}, y[3] = {-7.0, -7.0, -7.0}, z[3] = {-7.0, -7.0, -7.0};
        CHECK(ld_density_scores(d, 3, sums.data(), mask & 1 ? x : nullptr, mask & 2 ? y : nullptr, mask & 4 ? z : nullptr) == LD_OK);
        CHECK((mask & 1 ? x[2] == cc[2] : x[2] == -7.0) && (mask & 2 ? y[2] == ccm[2] : y[2] == -7.0) && (mask & 4 ? z[2] == inside[2] : z[2] == -7.0));
    }
    const ld_density_sums nothing = {0, 0, 0, 0, 0, 0};
    CHECK(ld_density_scores(d, 1, &nothing, cc, ccm, inside) == LD_OK && cc[0] == 0.0 && ccm[0] == 0.0 && inside[0] == 0.0);
    CHECK(ld_density_scores(d, 1, nullptr, cc, ccm, inside) == LD_ERR_INVALID && ld_density_scores(d, 0, nullptr, cc, ccm, inside) == LD_OK);
    CHECK(ld_density_scores(nullptr, 1, &nothing, cc, ccm, inside) == LD_ERR_INVALID);

    // refusals: the outputs keep their fill
    std::vector<ld_density_sums> guard = filled(3);
    std::fill(grid.begin(), grid.end(), FILL);
    double bad[3 * 7];
    std::memcpy(bad, poses, sizeof bad);
    bad[8] = NAN;
    CHECK(ld_complex_density_fit(c, d, 3, bad, 7, 300, guard.data()) == LD_ERR_INVALID && ld_complex_simulate_density(c, d, 3, bad, 7, 300, grid.data()) == LD_ERR_INVALID);
    std::memcpy(bad, poses, sizeof bad);
    bad[17] = 0.0;
    CHECK(ld_complex_density_fit(c, d, 3, bad, 7, 300, guard.data()) == LD_ERR_INVALID);
    bad[17] = 1.0, bad[14] = 1.1e6;
    CHECK(ld_complex_density_fit(c, d, 3, bad, 7, 300, guard.data()) == LD_ERR_INVALID);
    CHECK(ld_complex_density_fit(c, d, 3, poses, 6, 300, guard.data()) == LD_ERR_INVALID && ld_complex_density_fit(c, d, 3, poses, 7, 299, guard.data()) == LD_ERR_INVALID);
    CHECK(ld_complex_density_fit(c, d, 3, poses, 7, 15001, guard.data()) == LD_ERR_INVALID && ld_complex_density_fit(c, d, 3, nullptr, 7, 300, guard.data()) == LD_ERR_INVALID);
    CHECK(ld_complex_density_fit(c, d, 3, poses, 7, 300, nullptr) == LD_ERR_INVALID && ld_complex_density_fit(c, nullptr, 3, poses, 7, 300, guard.data()) == LD_ERR_INVALID);
    CHECK(ld_complex_density_fit(nullptr, d, 3, poses, 7, 300, guard.data()) == LD_ERR_INVALID);
    CHECK(ld_complex_density_fit(c, d, 3, poses, 7, 5000, guard.data()) == LD_ERR_INVALID);   // a support of 20.4 A on voxels of 1 A
    CHECK(sums_filled(guard) && grid == std::vector<uint32_t>(6, FILL));
    CHECK(ld_complex_density_fit(c, d, 0, nullptr, 7, 300, nullptr) == LD_OK && ld_complex_simulate_density(c, d, 0, nullptr, 7, 300, nullptr) == LD_OK);
    ld_density_destroy(d);
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
    const std::string dir = golden + "/1czy/";
    const std::vector<double> rec_nm = ld::read_npy_f64(dir + "lightdock_rec.nm.npy"), lig_nm = ld::read_npy_f64(dir + "lightdock_lig.nm.npy");
    const std::string rec = dir + "lightdock_1czy_protein.pdb", lig = dir + "lightdock_1czy_peptide.pdb";
    ld_complex *a = ld_complex_create(rec.c_str(), lig.c_str(), nullptr, 0, 0, lig_nm.data(), lig_nm.size(), 10);
    ld_complex *b = ld_complex_create(rec.c_str(), lig.c_str(), rec_nm.data(), rec_nm.size(), 10, lig_nm.data(), lig_nm.size(), 10);
    CHECK(a != nullptr && b != nullptr);
    if (!a || !b) return;
    const size_t n = 3;
    const std::vector<double> p[3] = {gso_pose(dir + "swarm_2/gso_100.out", 74), gso_pose(dir + "swarm_0/gso_100.out", 0), gso_pose(dir + "swarm_9/gso_100.out", 199)};
    std::vector<double> rigid_rec(n * 17, 0.0), flexible(n * 29, 0.0);   // a stride of 29 > 27
    for (size_t i = 0; i < n; i++) {
        CHECK(p[i].size() == 27);
        if (p[i].size() != 27) return;
        std::copy(p[i].begin(), p[i].begin() + 7, &rigid_rec[i * 17]);
        std::copy(p[i].begin() + 17, p[i].end(), &rigid_rec[i * 17 + 7]);
        std::copy(p[i].begin(), p[i].begin() + 7, &flexible[i * 29]);
        std::copy(p[i].begin() + 17, p[i].end(), &flexible[i * 29 + 17]);
    }
    // a small map of 6 A voxels around the receptor: 17 x 9 x 18, so two bricks on x and on z, one of them a single voxel deep
    const uint32_t dims[3] = {17, 9, 18}, step[3] = {6000, 5500, 6000};
    const int32_t origin[3] = {-20000, -10000, -30000};
    std::vector<float> rho(17 * 9 * 18);
    for (size_t v = 0; v < rho.size(); v++) rho[v] = (float)((v * 2654435761u) % 1000) - 300.0f;
    ld_density *d = ld_density_create(rho.data(), dims, origin, step, 0.0);
    CHECK(d != nullptr);
    if (!d) return;
    const size_t N = rho.size();
    std::vector<uint32_t> E(N);
    CHECK(ld_density_voxels(d, E.data()) == LD_OK);
    std::vector<ld_density_sums> sa = filled(n), sb = filled(n), pieces = filled(n);
    std::vector<uint32_t> ga(n * N, FILL), gb(n * N, FILL);
    const uint32_t sigma = 2250;
    CHECK(ld_complex_density_fit(a, d, n, rigid_rec.data(), 17, sigma, sa.data()) == LD_OK);
    CHECK(ld_complex_density_fit(b, d, n, flexible.data(), 29, sigma, sb.data()) == LD_OK);
    CHECK(ld_complex_simulate_density(a, d, n, rigid_rec.data(), 17, sigma, ga.data()) == LD_OK);
    CHECK(ld_complex_simulate_density(b, d, n, flexible.data(), 29, sigma, gb.data()) == LD_OK && ga == gb);
    for (size_t i = 0; i < n; i++) {
        CHECK(same(sa[i], sb[i]) && sa[i].reserved == 0);
        uint64_t s = 0, ss = 0, se = 0, in = 0;
        for (size_t v = 0; v < N; v++) {
            const uint64_t x = ga[i * N + v];
            s += x, ss += x * x, se += x * E[v], in += E[v] ? x : 0;
        }
        CHECK(s == sa[i].s && ss == sa[i].ss && se == sa[i].se && in == sa[i].inside_sum && s > 0);
    }
    CHECK(!same(sa[0], sa[1]));
    double ms = -1.0;
    CHECK(ld_complex_last_kernel_ms(a, &ms) == LD_OK && ms == 0.0);
    CHECK(ld_complex_density_chunk(a, 1) == LD_OK && ld_complex_density_chunk(nullptr, 1) == LD_ERR_INVALID);
    CHECK(ld_complex_density_fit(a, d, n, rigid_rec.data(), 17, sigma, pieces.data()) == LD_OK);
    for (size_t i = 0; i < n; i++) CHECK(same(pieces[i], sa[i]));
    CHECK(ld_complex_density_chunk(b, 2) == LD_OK && ld_complex_simulate_density(b, d, n, flexible.data(), 29, sigma, gb.data()) == LD_OK && ga == gb);
    CHECK(ld_complex_density_chunk(a, 0) == LD_OK && ld_complex_density_chunk(b, 0) == LD_OK);
    ld_density_destroy(d);
    ld_complex_destroy(a);
    ld_complex_destroy(b);
}

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: emfit_check <tests/golden> <scratch dir>\n");
        return 2;
    }
    maps_and_tables();
    by_hand(argv[2]);
    czy(argv[1]);
    std::printf("emfit_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
