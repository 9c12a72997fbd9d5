// prepare_check.cpp -- driver of the sanitizer build of the run-preparation path (`make asan-prepare`;
// tests/test_asan_prepare.py): ld_swarm_diameter2 / ld_swarm_shell / ld_swarm_centres / ld_initial_poses / ld_prepare_pdb
// through the C ABI against tests/asan/hip_stub.cpp and tests/asan/hip_stub_prepare.cpp (device memory = host memory; the
// launches do the kernels' work in plain C++ from the shared predicates).  The answers are checked against the rule as this
// file states it itself: every lattice node against every atom, farthest-point sampling by a plain loop.
//   usage: prepare_check <tests/golden> <scratch dir>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#define CHECK_PROGRAM "prepare_check"
#include "check.hpp"

typedef std::vector<int32_t> Ints;

static long long floor_div(long long a, long long b) {
    long long q = a / b;
    if (a % b != 0 && ((a < 0) != (b < 0))) q--;
    return q;
}

// The rule, node by node.
static Ints shell_by_hand(const Ints &atoms, const std::vector<uint8_t> &bead, int h, uint64_t *nodes) {
    const size_t n = atoms.size() / 4;
    long long lo[3], hi[3], e_max = 0;
    for (size_t a = 0; a < n; a++) e_max = std::max<long long>(e_max, atoms[4 * a + 3]);
    for (int c = 0; c < 3; c++) {
        long long mn = atoms[c], mx = atoms[c];
        for (size_t a = 0; a < n; a++) {
            mn = std::min<long long>(mn, atoms[4 * a + c]);
            mx = std::max<long long>(mx, atoms[4 * a + c]);
        }
        lo[c] = floor_div(mn - e_max - h, h);
        hi[c] = -floor_div(-(mx + e_max + h), h);
    }
    *nodes = (uint64_t)((hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1));
    Ints out;
    for (long long i = lo[0]; i <= hi[0]; i++)
        for (long long j = lo[1]; j <= hi[1]; j++)
            for (long long k = lo[2]; k <= hi[2]; k++) {
                const long long p[3] = {i * h, j * h, k * h};
                bool outside = true, near = false;
                for (size_t a = 0; a < n; a++) {
                    long long d2 = 0;
                    for (int c = 0; c < 3; c++) d2 += (p[c] - atoms[4 * a + c]) * (p[c] - atoms[4 * a + c]);
                    const long long E = atoms[4 * a + 3];
                    if (d2 < E * E) outside = false;
                    if (!(bead.size() && bead[a]) && d2 < (E + h) * (E + h)) near = true;
                }
                if (outside && near)
                    for (int c = 0; c < 3; c++) out.push_back((int32_t)p[c]);
            }
    return out;
}

static void centres_by_hand(const Ints &p, size_t most, long long cover, std::vector<uint32_t> *index, std::vector<uint64_t> *gap2) {
    const size_t n = p.size() / 3;
    std::vector<long long> value(n), gap(n, INT64_MAX);
    for (size_t i = 0; i < n; i++) value[i] = (long long)p[3 * i] * p[3 * i] + (long long)p[3 * i + 1] * p[3 * i + 1] + (long long)p[3 * i + 2] * p[3 * i + 2];
    while (index->size() < std::min(most, n)) {
        size_t at = 0;
        for (size_t i = 1; i < n; i++)
            if (value[i] > value[at]) at = i;
        if (value[at] < 0 || (!index->empty() && cover > 0 && value[at] <= cover * cover)) break;
        index->push_back((uint32_t)at);
        gap2->push_back((uint64_t)value[at]);
        for (size_t i = 0; i < n; i++) {
            long long d2 = 0;
            for (int c = 0; c < 3; c++) d2 += (long long)(p[3 * i + c] - p[3 * at + c]) * (p[3 * i + c] - p[3 * at + c]);
            gap[i] = gap[i] < 0 ? -1 : std::min(gap[i], d2);
        }
        gap[at] = -1;
        value = gap;
    }
}

// The two calls of ld_swarm_shell; checks them against the rule by hand.
static Ints shell_checked(const Ints &atoms, const std::vector<uint8_t> &bead, int h) {
    uint64_t nodes_want = 0, nodes = 0;
    const Ints want = shell_by_hand(atoms, bead, h, &nodes_want);
    size_t count = 99999;
    const uint8_t *flags = bead.empty() ? nullptr : bead.data();
    CHECK(ld_swarm_shell(atoms.data(), flags, atoms.size() / 4, h, nullptr, 0, &count, &nodes) == LD_OK);   // count only
    CHECK(count == want.size() / 3 && nodes == nodes_want);
    Ints got(3 * count + 3, -7);
    size_t again = 0;
    CHECK(ld_swarm_shell(atoms.data(), flags, atoms.size() / 4, h, got.data(), count, &again, nullptr) == LD_OK);
    CHECK(again == count && got[3 * count] == -7 && got[3 * count + 2] == -7);
    got.resize(3 * count);
    CHECK(got == want);
    if (count > 0) {   // a cap that is too small: the count is reported, the nodes are not touched
        Ints small(3 * count, -7);
        size_t reported = 0;
        CHECK(ld_swarm_shell(atoms.data(), flags, atoms.size() / 4, h, small.data(), count - 1, &reported, &nodes) == LD_ERR_INVALID);
        CHECK(reported == count && small == Ints(3 * count, -7) && nodes == nodes_want);
    }
    return got;
}

static void centres_checked(const Ints &points, size_t most, int cover) {
    std::vector<uint32_t> want_index;
    std::vector<uint64_t> want_gap2;
    centres_by_hand(points, most, cover, &want_index, &want_gap2);
    const size_t room = std::min(most, points.size() / 3);
    std::vector<uint32_t> index(room + 1, 77u);
    std::vector<uint64_t> gap2(room + 1, 77u);
    size_t n = 99999;
    CHECK(ld_swarm_centres(points.data(), points.size() / 3, most, cover, index.data(), gap2.data(), &n) == LD_OK);
    CHECK(n == want_index.size() && index[room] == 77u && gap2[room] == 77u);
    index.resize(n);
    gap2.resize(n);
    CHECK(index == want_index && gap2 == want_gap2);
    for (size_t k = 2; k < gap2.size(); k++) CHECK(gap2[k] <= gap2[k - 1]);
}

static void small_shapes() {
    shell_checked({0, 0, 0, 4700}, {}, 2000);                                  // one atom
    shell_checked({0, 0, 0, 4700, 2500, 300, -100, 4550}, {}, 2000);
    shell_checked({-50123, -47001, -39999, 4700, -52123, -48001, -41999, 4520}, {}, 2000);
    shell_checked({0, 0, 0, 4700, 5000, 0, 0, 5000}, {0, 1}, 2000);            // a bead beside an atom
    CHECK(shell_checked({0, 0, 0, 4700, 5000, 0, 0, 5000}, {1, 1}, 2000).empty());   // beads only: none, and no error
    shell_checked({2000000, -2000000, 2000000, 4700}, {}, 2000);
    shell_checked({2000000, 2000000, 2000000, 600000, -2000000, -2000000, -2000000, 600000}, {}, 500000);
    double ms = -1.0;
    CHECK(ld_setup_last_kernel_ms(&ms) == LD_OK && ms == 0.0);
    CHECK(ld_setup_last_kernel_ms(nullptr) == LD_ERR_INVALID);

    uint64_t d2 = 7;
    const Ints one = {5, -7, 9}, three = {0, 0, 0, 3, 4, 12, -2000000, 2000000, -2000000};
    CHECK(ld_swarm_diameter2(one.data(), 1, &d2) == LD_OK && d2 == 0);
    CHECK(ld_swarm_diameter2(three.data(), 2, &d2) == LD_OK && d2 == 169);
    CHECK(ld_swarm_diameter2(three.data(), 3, &d2) == LD_OK && d2 == 2000003ull * 2000003ull + 1999996ull * 1999996ull + 2000012ull * 2000012ull);

    Ints cube, scattered;
    for (int i = -1; i <= 1; i++)
        for (int j = -1; j <= 1; j++)
            for (int k = -1; k <= 1; k++) cube.insert(cube.end(), {2000 * i, 2000 * j, 2000 * k});
    unsigned state = 2463534242u;
    for (int i = 0; i < 3 * 700; i++) {   // 700 lattice points of a 9^3 box: two workgroups, duplicates
        state ^= state << 13;
        state ^= state >> 17;
        state ^= state << 5;
        scattered.push_back(2000 * ((int)(state % 9u) - 4));
    }
    centres_checked(cube, 27, 0);
    centres_checked(cube, 1000, 0);
    centres_checked(cube, 27, 2000);
    centres_checked(one, 3, 0);
    centres_checked({5, -7, 9, 5, -7, 9000}, 2, 9000);
    centres_checked(scattered, 700, 0);
    centres_checked(scattered, 90, 3000);
}

static void refusals() {
    Ints out(12, -7);
    size_t count = 4321;
    uint64_t nodes = 8765, d2 = 7;
    auto shell_refused = [&](const Ints &atoms, int h, const char *word) {
        const int rc = ld_swarm_shell(atoms.data(), nullptr, atoms.size() / 4, h, out.data(), 4, &count, &nodes);
        return rc == LD_ERR_INVALID && count == 4321 && nodes == 8765 && out == Ints(12, -7) && std::strstr(ld_last_error(), word) != nullptr;
    };
    CHECK(shell_refused({0, 0, 0, 4700}, 0, "spacing"));
    CHECK(shell_refused({0, 0, 0, 4700}, 1000001, "spacing"));
    CHECK(shell_refused({0, 0, 0, 0}, 2000, "extent"));
    CHECK(shell_refused({0, 0, 0, 4000001}, 2000, "extent"));
    CHECK(shell_refused({2000001, 0, 0, 4700}, 2000, "beyond"));
    CHECK(shell_refused({0, 0, -2000001, 4700}, 2000, "beyond"));
    CHECK(shell_refused({2000000, 2000000, 2000000, 4700, -2000000, -2000000, -2000000, 4700}, 2000, "spacing"));   // 8e9 nodes
    CHECK(shell_refused({0, 0, 0, 4700}, 1, "spacing"));                                                            // 9401^3 nodes
    const Ints atom = {0, 0, 0, 4700};
    CHECK(ld_swarm_shell(atom.data(), nullptr, 0, 2000, out.data(), 4, &count, &nodes) == LD_ERR_INVALID && count == 4321);
    CHECK(ld_swarm_shell(nullptr, nullptr, 1, 2000, out.data(), 4, &count, &nodes) == LD_ERR_INVALID && count == 4321);
    CHECK(ld_swarm_shell(atom.data(), nullptr, 1, 2000, out.data(), 4, nullptr, &nodes) == LD_ERR_INVALID && out == Ints(12, -7));

    const Ints far = {0, 2000001, 0};
    CHECK(ld_swarm_diameter2(far.data(), 1, &d2) == LD_ERR_INVALID && d2 == 7);
    CHECK(ld_swarm_diameter2(atom.data(), 0, &d2) == LD_ERR_INVALID && d2 == 7);
    CHECK(ld_swarm_diameter2(nullptr, 1, &d2) == LD_ERR_INVALID && ld_swarm_diameter2(atom.data(), 1, nullptr) == LD_ERR_INVALID);

    std::vector<uint32_t> index(4, 9u);
    std::vector<uint64_t> gap2(4, 9u);
    size_t n = 55;
    auto centres_refused = [&](const int32_t *p, size_t points, size_t most, int cover) {
        const int rc = ld_swarm_centres(p, points, most, cover, index.data(), gap2.data(), &n);
        return rc == LD_ERR_INVALID && n == 55 && index == std::vector<uint32_t>(4, 9u) && gap2 == std::vector<uint64_t>(4, 9u);
    };
    CHECK(centres_refused(atom.data(), 1, 0, 0));
    CHECK(centres_refused(atom.data(), 1, 4, -1));
    CHECK(centres_refused(far.data(), 1, 4, 0));
    CHECK(centres_refused(atom.data(), ((size_t)1 << 22) + 1, 4, 0));
    CHECK(centres_refused(nullptr, 1, 4, 0));
    CHECK(ld_swarm_centres(atom.data(), 1, 4, 0, nullptr, gap2.data(), &n) == LD_ERR_INVALID);
    CHECK(ld_swarm_centres(atom.data(), 1, 4, 0, index.data(), gap2.data(), nullptr) == LD_ERR_INVALID);
    CHECK(ld_swarm_centres(nullptr, 0, 4, 0, index.data(), gap2.data(), &n) == LD_OK && n == 0);
}

static std::vector<std::string> atom_records(const std::string &path) {
    std::vector<std::string> out;
    std::ifstream in(path);
    std::string line;
    while (std::getline(in, line))
        if (line.compare(0, 6, "ATOM  ") == 0 || line.compare(0, 6, "HETATM") == 0) out.push_back(line);
    return out;
}

static std::string slurp(const std::string &path) {
    std::ifstream in(path, std::ios::binary);
    return std::string((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

static void on_files(const std::string &golden, const std::string &scratch) {
    // the cleaner: the golden files come back as they are; flags; refusals that write nothing
    const std::string peptide = golden + "/1czy/lightdock_1czy_peptide.pdb", protein = golden + "/1czy/lightdock_1czy_protein.pdb";
    size_t atoms = 0;
    double centre[3] = {9, 9, 9};
    CHECK(ld_prepare_pdb(peptide.c_str(), (scratch + "/peptide.pdb").c_str(), 0, &atoms, centre) == LD_OK);
    CHECK(atoms == 53 && std::fabs(centre[0]) < 0.0005 && slurp(scratch + "/peptide.pdb") == slurp(peptide));
    CHECK(ld_prepare_pdb(protein.c_str(), (scratch + "/protein.pdb").c_str(), 7, nullptr, nullptr) == LD_OK);
    CHECK(slurp(scratch + "/protein.pdb") == slurp(protein));
    const char *rest = "  1.00  0.00           C\n";
    std::string text = atom_line(1, "N", "ALA", 'A', 1, 10.0, 0.0, 0.001, "  1.00  0.00           N\n") +
                       atom_line(2, "CA", "ALA", 'A', 1, 11.0, 1.0, 0.002, rest) + atom_line(3, "H", "ALA", 'A', 1, 12.0, 2.0, 0.0, "  1.00  0.00           H\n") +
                       atom_line(4, "OXT", "ALA", 'A', 1, 13.0, 3.0, 0.0, "  1.00  0.00           O\n") +
                       atom_line(5, "O", "HOH", 'A', 2, 14.0, 4.0, 0.0, "  1.00  0.00           O\n") +
                       atom_line(6, "BJ", "MMB", 'M', 3, -15.0, 5.0, 0.0, "\n") + "TER\n" + atom_line(7, "HB1", "ALA", 'A', 4, 16.0, 6.0, 0.0, "\n");
    put(scratch + "/hand.pdb", text);
    const size_t kept[] = {3, 5, 4, 6, 4, 6, 5, 7};   // by flags 0 .. 7: hydrogens are two records, OXT and the water one each
    for (int flags = 0; flags < 8; flags++) {
        CHECK(ld_prepare_pdb((scratch + "/hand.pdb").c_str(), (scratch + "/hand_out.pdb").c_str(), flags, &atoms, centre) == LD_OK);
        CHECK(atoms == kept[flags] && atom_records(scratch + "/hand_out.pdb").size() == kept[flags]);
    }
    put(scratch + "/short.pdb", text + std::string("ATOM      8  CB  ALA A   5      17.000   7.000\n"));
    CHECK(ld_prepare_pdb((scratch + "/short.pdb").c_str(), (scratch + "/never.pdb").c_str(), 0, &atoms, centre) == LD_ERR_IO);
    put(scratch + "/only_h.pdb", atom_line(3, "H", "ALA", 'A', 1, 12.0, 2.0, 0.0, "  1.00  0.00           H\n"));
    CHECK(ld_prepare_pdb((scratch + "/only_h.pdb").c_str(), (scratch + "/never.pdb").c_str(), 0, &atoms, centre) == LD_ERR_INVALID);
    CHECK(ld_prepare_pdb((scratch + "/none.pdb").c_str(), (scratch + "/never.pdb").c_str(), 0, &atoms, centre) == LD_ERR_IO);
    CHECK(ld_prepare_pdb(nullptr, (scratch + "/never.pdb").c_str(), 0, &atoms, centre) == LD_ERR_INVALID);
    CHECK(ld_prepare_pdb((scratch + "/hand.pdb").c_str(), (scratch + "/no_such_dir/x.pdb").c_str(), 0, &atoms, centre) == LD_ERR_IO);
    CHECK(slurp(scratch + "/never.pdb").empty());

    // a 1czy subset: the peptide's diameter, the shell of the receptor's first 40 atoms (carbon radii), its centres
    Ints lig, rec;
    for (const std::string &line : atom_records(peptide))
        for (int c = 0; c < 3; c++) lig.push_back((int32_t)std::llrint(std::atof(line.substr(30 + 8 * c, 8).c_str()) * 1000.0));
    uint64_t d2 = 0, by_hand = 0;
    CHECK(ld_swarm_diameter2(lig.data(), lig.size() / 3, &d2) == LD_OK);
    for (size_t i = 0; i < lig.size() / 3; i++)
        for (size_t j = 0; j < i; j++) {
            uint64_t s = 0;
            for (int c = 0; c < 3; c++) s += (uint64_t)((long long)(lig[3 * i + c] - lig[3 * j + c]) * (lig[3 * i + c] - lig[3 * j + c]));
            by_hand = std::max(by_hand, s);
        }
    const int D = (int)(std::floor(std::sqrt((double)d2)) / 4);
    CHECK(d2 == by_hand && D == 4697);
    const std::vector<std::string> records = atom_records(protein);
    for (size_t a = 0; a < 40 && a < records.size(); a++) {
        for (int c = 0; c < 3; c++) rec.push_back((int32_t)std::llrint(std::atof(records[a].substr(30 + 8 * c, 8).c_str()) * 1000.0));
        rec.push_back(1700 + D);
    }
    const Ints candidates = shell_checked(rec, {}, 2000);
    CHECK(candidates.size() / 3 > 100);
    centres_checked(candidates, 400, 10000);
    centres_checked(candidates, 12, 0);
}

static void poses() {
    const double centre[3] = {12.5, -7.25, 30.0}, rec[6] = {3.25, -1.5, 7.125, -8.0, 2.75, 0.5}, lig[3] = {1.0, 2.0, -0.5};
    std::vector<double> rows(8 * 30 + 1, -7.0), again(30, -7.0);
    std::vector<uint64_t> draws(9, 77u);
    CHECK(ld_initial_poses(324324, 8, 3, 0, 8, centre, 10.0, nullptr, 0, nullptr, 0, 11, 12, rows.data(), draws.data()) == LD_OK);
    CHECK(rows[8 * 30] == -7.0 && draws[8] == 77u);
    for (size_t g = 0; g < 8; g++) {
        const double *r = &rows[30 * g];
        const double d = std::sqrt((r[0] - centre[0]) * (r[0] - centre[0]) + (r[1] - centre[1]) * (r[1] - centre[1]) + (r[2] - centre[2]) * (r[2] - centre[2]));
        CHECK(d <= 10.0 * (1.0 + 1e-15) && std::fabs(std::sqrt(r[3] * r[3] + r[4] * r[4] + r[5] * r[5] + r[6] * r[6]) - 1.0) < 1e-15);
        CHECK(draws[g] >= 3 + 4 + 24);
        for (int k = 7; k < 30; k++) CHECK(std::isfinite(r[k]) && std::fabs(r[k]) < 10.0);
        CHECK(ld_initial_poses(324324, 8, 3, g, 1, centre, 10.0, nullptr, 0, nullptr, 0, 11, 12, again.data(), nullptr) == LD_OK);
        CHECK(std::memcmp(again.data(), r, 30 * sizeof(double)) == 0);
    }
    std::vector<double> seven(7 * 8, -7.0);
    CHECK(ld_initial_poses(1, 8, 0, 0, 8, centre, 10.0, rec, 2, lig, 1, 0, 0, seven.data(), draws.data()) == LD_OK);
    for (size_t g = 0; g < 8; g++) CHECK(draws[g] >= 5 && std::fabs(std::sqrt(seven[7 * g + 3] * seven[7 * g + 3] + seven[7 * g + 4] * seven[7 * g + 4] +
                                                                             seven[7 * g + 5] * seven[7 * g + 5] + seven[7 * g + 6] * seven[7 * g + 6]) - 1.0) < 1e-15);
    const std::vector<double> before = seven;
    const double bad_centre[3] = {0.0, NAN, 0.0}, bad_point[3] = {INFINITY, 0.0, 0.0};
    CHECK(ld_initial_poses(1, 8, 0, 6, 3, centre, 10.0, nullptr, 0, nullptr, 0, 0, 0, seven.data(), nullptr) == LD_ERR_INVALID);
    CHECK(ld_initial_poses(1, 0, 0, 0, 1, centre, 10.0, nullptr, 0, nullptr, 0, 0, 0, seven.data(), nullptr) == LD_ERR_INVALID);
    CHECK(ld_initial_poses(1, 8, 0, 0, 8, centre, -1.0, nullptr, 0, nullptr, 0, 0, 0, seven.data(), nullptr) == LD_ERR_INVALID);
    CHECK(ld_initial_poses(1, 8, 0, 0, 8, bad_centre, 10.0, nullptr, 0, nullptr, 0, 0, 0, seven.data(), nullptr) == LD_ERR_INVALID);
    CHECK(ld_initial_poses(1, 8, 0, 0, 8, centre, 10.0, bad_point, 1, lig, 1, 0, 0, seven.data(), nullptr) == LD_ERR_INVALID);
    CHECK(ld_initial_poses(1, 8, 0, 0, 8, centre, 10.0, nullptr, 1, lig, 1, 0, 0, seven.data(), nullptr) == LD_ERR_INVALID);
    CHECK(ld_initial_poses(1, 8, 0, 0, 8, centre, 10.0, nullptr, 0, nullptr, 0, 5000, 0, seven.data(), nullptr) == LD_ERR_INVALID);
    CHECK(ld_initial_poses(1, 8, 0, 0, 8, nullptr, 10.0, nullptr, 0, nullptr, 0, 0, 0, seven.data(), nullptr) == LD_ERR_INVALID);
    CHECK(ld_initial_poses(1, 8, 0, 0, 8, centre, 10.0, nullptr, 0, nullptr, 0, 0, 0, nullptr, nullptr) == LD_ERR_INVALID);
    CHECK(seven == before);
    CHECK(ld_initial_poses(1, 8, 0, 0, 0, centre, 10.0, nullptr, 0, nullptr, 0, 0, 0, nullptr, nullptr) == LD_OK);
}

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: prepare_check <tests/golden> <scratch dir>\n");
        return 2;
    }
    small_shapes();
    refusals();
    on_files(argv[1], argv[2]);
    poses();
    std::printf("prepare_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
