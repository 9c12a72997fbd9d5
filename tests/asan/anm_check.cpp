// anm_check.cpp -- driver of the sanitizer build of the normal-mode path (`make asan-anm`; tests/test_asan_anm.py):
// ld_anm_nodes / ld_anm_modes_xyz / ld_anm_modes through the C ABI against tests/asan/hip_stub.cpp and
// tests/asan/hip_stub_anm.cpp (device memory = host memory; the launches do the kernels' work in plain C++ with the shared
// rules of kernels/anm.hpp).  The answers are checked against what defines them: the modes are orthonormal, H v = lambda v
// with a Hessian this file builds itself, the eigenvalues ascend, the sign rule holds.
//   usage: anm_check <tests/golden> <scratch dir>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#define CHECK_PROGRAM "anm_check"
#include "check.hpp"

static const char *const kRest = "  1.00  0.00\n";

// The ATOM / HETATM coordinates of a file, in file order.
static std::vector<double> file_xyz(const std::string &path) {
    std::vector<double> xyz;
    std::ifstream in(path);
    std::string line;
    while (std::getline(in, line))
        if (line.size() >= 54 && (line.compare(0, 6, "ATOM  ") == 0 || line.compare(0, 6, "HETATM") == 0))
            for (int c = 0; c < 3; c++) xyz.push_back(std::atof(line.substr(30 + 8 * c, 8).c_str()));
    return xyz;
}

// H of the header's rule, row-major n x n.
static std::vector<double> hessian(const std::vector<double> &xyz, double cutoff) {
    const size_t m = xyz.size() / 3, n = 3 * m;
    std::vector<double> H(n * n, 0.0);
    for (size_t i = 0; i < m; i++)
        for (size_t j = 0; j < m; j++) {
            if (i == j) continue;
            const double d[3] = {xyz[3 * j] - xyz[3 * i], xyz[3 * j + 1] - xyz[3 * i + 1], xyz[3 * j + 2] - xyz[3 * i + 2]};
            const double d2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
            if (!(d2 > 0.0 && d2 <= cutoff * cutoff)) continue;
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 3; b++) {
                    H[(3 * i + a) * n + 3 * j + b] = -d[a] * d[b] / d2;
                    H[(3 * i + a) * n + 3 * i + b] += d[a] * d[b] / d2;
                }
        }
    return H;
}

// k unit node modes against their definition; tol: absolute, for residuals and products of unit vectors.
static void check_modes(const std::vector<double> &xyz, size_t k, const std::vector<double> &modes, const std::vector<double> &eig,
                        double tol) {
    const size_t n = xyz.size();
    const std::vector<double> H = hessian(xyz, 15.0);
    for (size_t r = 0; r < k; r++) {
        const double *v = &modes[r * n];
        CHECK(eig[r] >= 1e-6 && (r == 0 || eig[r] >= eig[r - 1]));
        double worst = 0.0, largest = 0.0;
        size_t at = 0;
        for (size_t i = 0; i < n; i++) {
            double hv = 0.0;
            for (size_t j = 0; j < n; j++) hv += H[i * n + j] * v[j];
            worst = std::fmax(worst, std::fabs(hv - eig[r] * v[i]));
            if (std::fabs(v[i]) > largest) {
                largest = std::fabs(v[i]);
                at = i;
            }
        }
        CHECK(worst < tol);
        CHECK(v[at] > 0.0);
        for (size_t s = 0; s <= r; s++) {
            double dot = 0.0;
            for (size_t i = 0; i < n; i++) dot += v[i] * modes[s * n + i];
            CHECK(std::fabs(dot - (s == r ? 1.0 : 0.0)) < tol);
        }
    }
}

// Points that hold together: a jittered helix, 3.8 A between neighbours.
static std::vector<double> chain(size_t m) {
    std::vector<double> xyz;
    unsigned state = 12345u;
    for (size_t i = 0; i < m; i++) {
        state = state * 1664525u + 1013904223u;
        const double jitter = ((state >> 8) & 0xffff) / 65536.0 - 0.5;
        xyz.push_back(5.0 * std::cos(1.7 * i) + jitter);
        xyz.push_back(5.0 * std::sin(1.7 * i) - 0.5 * jitter);
        xyz.push_back(1.5 * i + 0.3 * jitter);
    }
    return xyz;
}

static void on_coordinates() {
    // n = 12 (even, every mode asked for), 15 and 21 (odd: a bye every step), 66 (even, past a wave)
    const size_t shapes[][2] = {{4, 6}, {5, 9}, {7, 10}, {22, 10}};
    for (const auto &shape : shapes) {
        const size_t m = shape[0], k = shape[1];
        std::vector<double> xyz = chain(m);
        if (m == 4) xyz = {0, 0, 0, 3.8, 0.2, 0, 1.1, 3.5, 0.4, 1.6, 1.2, 3.3};   // an irregular tetrahedron
        std::vector<double> modes(k * m * 3, -7.0), eig(k, -7.0);
        CHECK(ld_anm_modes_xyz(xyz.data(), m, k, 15.0, modes.data(), eig.data()) == LD_OK);
        check_modes(xyz, k, modes, eig, 1e-10);
        std::vector<double> again(k * m * 3, -7.0);
        CHECK(ld_anm_modes_xyz(xyz.data(), m, k, 15.0, again.data(), nullptr) == LD_OK);   // NULL eigenvalues_out
        CHECK(std::memcmp(again.data(), modes.data(), modes.size() * sizeof(double)) == 0);
    }
    double ms = -1.0;
    CHECK(ld_anm_last_kernel_ms(&ms) == LD_OK && ms == 0.0);
    CHECK(ld_anm_last_kernel_ms(nullptr) == LD_ERR_INVALID);
}

static bool untouched(const std::vector<double> &v) {
    for (double x : v)
        if (x != -7.0) return false;
    return true;
}

static void refusals(const std::string &scratch) {
    std::vector<double> modes(129 * 30 * 3, -7.0), eig(129, -7.0);
    const std::vector<double> ten = chain(10);
    auto refused = [&](const std::vector<double> &xyz, size_t m, size_t k, double cutoff) {
        const int rc = ld_anm_modes_xyz(xyz.data(), m, k, cutoff, modes.data(), eig.data());
        return rc == LD_ERR_INVALID && untouched(modes) && untouched(eig) && std::strlen(ld_last_error()) > 0;
    };
    CHECK(refused(chain(3), 3, 4, 15.0));    // 9 < 6 + 4
    CHECK(refused(chain(4), 4, 7, 15.0));    // 12 < 6 + 7
    CHECK(refused(ten, 10, 0, 15.0));
    CHECK(refused(ten, 10, 129, 15.0));
    CHECK(refused(std::vector<double>(3 * 4097, 0.0), 4097, 10, 15.0));
    for (double cutoff : {0.0, -15.0, (double)NAN, (double)INFINITY, 1e200}) CHECK(refused(ten, 10, 10, cutoff));
    std::vector<double> bad = ten;
    bad[17] = NAN;
    CHECK(refused(bad, 10, 10, 15.0));
    bad[17] = INFINITY;
    CHECK(refused(bad, 10, 10, 15.0));
    std::vector<double> apart = ten;   // two clusters 100 A apart: twelve zero modes
    for (size_t i = 0; i < 10; i++) {
        apart.push_back(ten[3 * i] + 100.0);
        apart.push_back(ten[3 * i + 1]);
        apart.push_back(ten[3 * i + 2]);
    }
    CHECK(refused(apart, 20, 10, 15.0));
    std::vector<double> line;          // collinear: nothing resists a bend
    for (int i = 0; i < 5; i++) {
        line.push_back(3.8 * i);
        line.push_back(0.0);
        line.push_back(0.0);
    }
    CHECK(refused(line, 5, 4, 15.0));
    CHECK(ld_anm_modes_xyz(nullptr, 10, 10, 15.0, modes.data(), eig.data()) == LD_ERR_INVALID);
    CHECK(ld_anm_modes_xyz(ten.data(), 10, 10, 15.0, nullptr, eig.data()) == LD_ERR_INVALID && untouched(eig));

    // files: a residue without a node atom is named; a file that is not there
    std::string text;
    const char *names[3] = {"N", "CA", "C"};
    for (int r = 0; r < 4; r++)
        for (int a = 0; a < 3; a++)
            text += atom_line(3 * r + a + 1, r == 2 && a == 1 ? "CB" : names[a], "ALA", 'A', r + 1, 3.8 * r + 0.5 * a, 1.0 * (r % 2), 0.7 * a * r, kRest);
    put(scratch + "/no_node.pdb", text);
    uint32_t nodes[8];
    size_t n_res = 99;
    CHECK(ld_anm_nodes((scratch + "/no_node.pdb").c_str(), nodes, &n_res) == LD_ERR_INVALID && n_res == 99);
    CHECK(std::strstr(ld_last_error(), "A.ALA.3") != nullptr);
    CHECK(ld_anm_modes((scratch + "/no_node.pdb").c_str(), 3, 15.0, 0.0, modes.data(), eig.data()) == LD_ERR_INVALID && untouched(modes));
    CHECK(std::strstr(ld_last_error(), "A.ALA.3") != nullptr);
    CHECK(ld_anm_modes((scratch + "/no_such.pdb").c_str(), 3, 15.0, 0.0, modes.data(), eig.data()) == LD_ERR_IO && untouched(modes));
    CHECK(ld_anm_nodes(nullptr, nodes, &n_res) == LD_ERR_INVALID && ld_anm_nodes((scratch + "/no_node.pdb").c_str(), nodes, nullptr) == LD_ERR_INVALID);
    CHECK(ld_anm_modes(nullptr, 3, 15.0, 0.0, modes.data(), eig.data()) == LD_ERR_INVALID);
}

static void on_files(const std::string &golden) {
    const struct {
        const char *file;
        size_t residues;
    } cases[] = {{"/1czy/lightdock_1czy_peptide.pdb", 7}, {"/2uuy/lightdock_2UUY_lig.pdb", 55}};
    for (const auto &c : cases) {
        const std::string path = golden + c.file;
        size_t n_res = 0;
        CHECK(ld_anm_nodes(path.c_str(), nullptr, &n_res) == LD_OK && n_res == c.residues);
        std::vector<uint32_t> nodes(n_res);
        CHECK(ld_anm_nodes(path.c_str(), nodes.data(), &n_res) == LD_OK);
        const std::vector<double> all = file_xyz(path);
        const size_t atoms = all.size() / 3, k = 10;
        std::vector<double> xyz;
        for (uint32_t a : nodes) {
            CHECK(a < atoms);
            if (a < atoms) xyz.insert(xyz.end(), all.begin() + 3 * a, all.begin() + 3 * a + 3);
        }
        std::vector<double> node_modes(k * n_res * 3), eig(k), modes(k * atoms * 3, -7.0), eig2(k), scaled(k * atoms * 3);
        CHECK(ld_anm_modes_xyz(xyz.data(), n_res, k, 15.0, node_modes.data(), eig.data()) == LD_OK);
        check_modes(xyz, k, node_modes, eig, 1e-10);
        CHECK(ld_anm_modes(path.c_str(), k, 15.0, 0.0, modes.data(), eig2.data()) == LD_OK);
        CHECK(eig == eig2);
        CHECK(ld_anm_modes(path.c_str(), k, 15.0, 0.5, scaled.data(), nullptr) == LD_OK);
        double inverse = 0.0;
        for (double e : eig) inverse += 1.0 / e;
        for (size_t r = 0; r < k; r++) {
            // unit over all atoms; a node's own atom carries the node mode up to one factor a mode; the amplitude rule
            double sum = 0.0, factor = 0.0, worst = 0.0, amp = 0.0;
            for (size_t i = 0; i < atoms * 3; i++) sum += modes[r * atoms * 3 + i] * modes[r * atoms * 3 + i];
            CHECK(std::fabs(sum - 1.0) < 1e-12);
            size_t top = 0;
            for (size_t i = 1; i < n_res * 3; i++)
                if (std::fabs(node_modes[r * n_res * 3 + i]) > std::fabs(node_modes[r * n_res * 3 + top])) top = i;
            factor = modes[(r * atoms + nodes[top / 3]) * 3 + top % 3] / node_modes[r * n_res * 3 + top];
            for (size_t i = 0; i < n_res * 3; i++)
                worst = std::fmax(worst, std::fabs(modes[(r * atoms + nodes[i / 3]) * 3 + i % 3] - factor * node_modes[r * n_res * 3 + i]));
            CHECK(factor > 0.0 && worst < 1e-14);
            const double want = 0.5 * std::sqrt((double)atoms) / std::sqrt(inverse) / std::sqrt(eig[r]);
            for (size_t i = 0; i < atoms * 3; i++) amp = std::fmax(amp, std::fabs(scaled[r * atoms * 3 + i] - want * modes[r * atoms * 3 + i]));
            CHECK(amp < 1e-14 * want);
        }
    }
}

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: anm_check <tests/golden> <scratch dir>\n");
        return 2;
    }
    on_coordinates();
    refusals(argv[2]);
    on_files(argv[1]);
    std::printf("anm_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
