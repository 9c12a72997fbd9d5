// assess_check.cpp -- driver of the sanitizer build of the model-quality path (`make asan-assess`; tests/test_asan_assess.py):
// ld_complex_set_reference / _reference_counts / _native_pairs / _assess through the C ABI against tests/asan/hip_stub.cpp and
// tests/asan/hip_stub_assess.cpp (device memory = host memory), and the f64 arithmetic after the integer sums
// (kernels/assess.hpp, host code too) on constructions whose answer is known.
//   usage: assess_check <tests/golden> <scratch dir>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#define CHECK_PROGRAM "assess_check"
#include "check.hpp"
#include "kernels/assess.hpp"

struct Point {
    long long x, y, z;
};

// The words of one fit set from points: what complex_assess_sums leaves.
static void set_words(const std::vector<Point> &model, const std::vector<Point> &ref, long long *w, long long sr[3], double *g_ref) {
    std::memset(w, 0, ld::kAssessSetWords * sizeof(long long));
    sr[0] = sr[1] = sr[2] = 0;
    ld::assess_wide ss = 0;
    for (size_t i = 0; i < model.size(); i++) {
        const long long m[3] = {model[i].x, model[i].y, model[i].z}, r[3] = {ref[i].x, ref[i].y, ref[i].z};
        for (int a = 0; a < 3; a++) {
            w[a] += m[a];
            w[3] += m[a] * m[a];
            sr[a] += r[a];
            ss += (ld::assess_wide)r[a] * r[a];
            for (int b = 0; b < 3; b++) w[4 + 3 * a + b] += m[a] * r[b];
        }
    }
    const ld::assess_wide n = (long long)ref.size();
    *g_ref = ld::assess_to_double(n * ss - ((ld::assess_wide)sr[0] * sr[0] + (ld::assess_wide)sr[1] * sr[1] + (ld::assess_wide)sr[2] * sr[2])) /
             (double)ref.size();
}

// RMSD in A of `model` on `ref` after their own best superposition.
static double fit_rmsd(const std::vector<Point> &model, const std::vector<Point> &ref, double q[4]) {
    long long w[ld::kAssessSetWords], sr[3];
    double g;
    set_words(model, ref, w, sr, &g);
    return std::sqrt(ld::assess_fit(w, (long long)ref.size(), sr, g, q)) / 1000.0;
}

static void numerics() {
    // a chiral set of four atoms, 1 .. 4 A apart
    const std::vector<Point> ref = {{0, 0, 0}, {1500, 0, 0}, {0, 2500, 0}, {300, 400, 3500}};
    double q[4];
    CHECK(fit_rmsd(ref, ref, q) < 1e-6 && std::fabs(std::fabs(q[0]) - 1.0) < 1e-12);
    // a turn of 180 degrees about each axis, then a translation: w = 0 in the rotation's quaternion
    for (int axis = 0; axis < 3; axis++) {
        std::vector<Point> model;
        for (const Point &p : ref) {
            const long long s[3] = {axis == 0 ? 1 : -1, axis == 1 ? 1 : -1, axis == 2 ? 1 : -1};
            model.push_back({s[0] * p.x + 1999000, s[1] * p.y - 1999000, s[2] * p.z + 7});
        }
        const double rmsd = fit_rmsd(model, ref, q);
        CHECK(std::isfinite(rmsd) && rmsd < 1e-5);
        CHECK(std::fabs(q[0]) < 1e-9 && std::fabs(std::fabs(q[1 + axis]) - 1.0) < 1e-9);
    }
    // the mirror image is not a fit
    std::vector<Point> mirror;
    for (const Point &p : ref) mirror.push_back({p.x, p.y, -p.z});
    const double m = fit_rmsd(mirror, ref, q);
    CHECK(std::isfinite(m) && m > 0.1);
    // all atoms of the model in one place, collinear atoms, three atoms: finite
    CHECK(std::isfinite(fit_rmsd({{5, 5, 5}, {5, 5, 5}, {5, 5, 5}, {5, 5, 5}}, ref, q)));
    const std::vector<Point> line = {{0, 0, 0}, {1000, 0, 0}, {2000, 0, 0}};
    CHECK(fit_rmsd(line, line, q) < 1e-6);
    CHECK(std::isfinite(fit_rmsd(line, {{0, 0, 0}, {0, 1000, 0}, {0, 2000, 1}}, q)));
    // a quarter turn about z with a known misfit: the model's last atom lifted by 1 A
    std::vector<Point> turned;
    for (const Point &p : ref) turned.push_back({-p.y, p.x, p.z});
    CHECK(fit_rmsd(turned, ref, q) < 1e-6 && std::fabs(std::fabs(q[3]) - std::sqrt(0.5)) < 1e-9);

    // L-RMSD: receptor = ref, ligand = one atom 1 A off after the receptor's superposition
    ld::AssessSolve k;
    long long w[ld::kAssessWords] = {};
    std::vector<Point> lig_ref = {{9000, 0, 0}, {9000, 1000, 0}}, lig_model = {{0, 9000, 0}, {-1000, 9000, 1000}};   // turned; the second 1 A up
    k.n_rec = 4, k.n_lig = 2, k.n_int = 4;
    set_words(turned, ref, w + ld::kAssessRec, k.sr_rec, &k.g_rec);
    set_words(turned, ref, w + ld::kAssessInt, k.sr_int, &k.g_int);
    double unused;
    set_words(lig_model, lig_ref, w + ld::kAssessLig, k.sr_lig, &unused);
    {   // the ligand's reference atoms about the receptor's centroid
        double g = 0;
        for (const Point &p : lig_ref) {
            const double d[3] = {p.x - k.sr_rec[0] / 4.0, p.y - k.sr_rec[1] / 4.0, p.z - k.sr_rec[2] / 4.0};
            g += d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        }
        k.g_lig = g;
    }
    double l, i;
    ld::assess_solve_pose(k, w, &l, &i);
    CHECK(i < 1e-6 && std::fabs(l - std::sqrt(0.5)) < 1e-6);   // sqrt((0 + 1) / 2)
}

// The columns of a record after its coordinates: occupancy, B-factor, the line end.
static const char *const kRest = "  1.00  0.00\n";

static void through_the_abi(const std::string &golden, const std::string &scratch) {
    const std::string rec = golden + "/1ppe/lightdock_1ppe_e.pdb", lig = golden + "/1ppe/lightdock_1ppe_i.pdb";
    ld_complex *c = ld_complex_create(rec.c_str(), lig.c_str(), nullptr, 0, 0, nullptr, 0, 0);
    CHECK(c != nullptr);
    if (!c) return;
    const size_t len = ld_complex_pose_len(c), stride = len + 3, n = 70000;   // more than a chunk of poses, more than the slots
    std::vector<double> poses(n * stride, 0.0);
    for (size_t i = 0; i < n; i++) poses[i * stride + 3] = 1.0;
    std::vector<uint32_t> kept(n, 0xA5A5A5A5u);
    std::vector<double> l(n, -7.0), r(n, -7.0);
    uint32_t counts[6] = {};

    // no reference yet
    CHECK(ld_complex_assess(c, 4, poses.data(), stride, kept.data(), l.data(), r.data()) == LD_ERR_INVALID);
    CHECK(ld_complex_reference_counts(c, counts) == LD_ERR_INVALID && ld_complex_native_pairs(c, kept.data()) == LD_ERR_INVALID);
    CHECK(kept[0] == 0xA5A5A5A5u && l[0] == -7.0 && r[0] == -7.0);

    // the model's own files as the reference
    CHECK(ld_complex_set_reference(c, rec.c_str(), lig.c_str(), 5.0, 10.0) == LD_OK);
    CHECK(ld_complex_reference_counts(c, counts) == LD_OK);
    CHECK(counts[0] == ld_complex_num_atoms(c, 0) && counts[1] == ld_complex_num_atoms(c, 1) && counts[2] > 0);
    CHECK(counts[3] >= 3 && counts[4] >= 1 && counts[5] >= 3 && counts[5] <= counts[3] + counts[4]);
    std::vector<uint32_t> pairs(2 * (size_t)counts[2]);
    CHECK(ld_complex_native_pairs(c, pairs.data()) == LD_OK);
    for (size_t p = 0; p < counts[2]; p++) {
        CHECK(pairs[2 * p] < ld_complex_num_residues(c, 0) && pairs[2 * p + 1] < ld_complex_num_residues(c, 1));
        if (p) CHECK(pairs[2 * p - 2] < pairs[2 * p] || (pairs[2 * p - 2] == pairs[2 * p] && pairs[2 * p - 1] < pairs[2 * p + 1]));
    }
    CHECK(ld_complex_assess(c, n, poses.data(), stride, kept.data(), l.data(), r.data()) == LD_OK);
    CHECK(kept[0] == counts[2] && kept[n - 1] == counts[2]);
    CHECK(l[0] >= 0.0 && l[0] < 1e-5 && r[0] >= 0.0 && r[0] < 1e-5 && l[n - 1] == l[0] && r[n - 1] == r[0]);   // the stub's model is the reference, moved
    CHECK(ld_complex_assess(c, 1, poses.data(), len, nullptr, nullptr, nullptr) == LD_OK);
    CHECK(ld_complex_assess(c, 1500, poses.data(), stride, nullptr, l.data(), nullptr) == LD_OK);
    CHECK(ld_complex_assess(c, 0, nullptr, len, nullptr, nullptr, nullptr) == LD_OK);
    double ms = -1.0;
    CHECK(ld_complex_last_kernel_ms(c, &ms) == LD_OK && ms == 0.0);

    // refusals at call time: nothing written
    std::fill(kept.begin(), kept.end(), 0xA5A5A5A5u);
    std::vector<double> bad(poses.begin(), poses.begin() + 4 * stride);
    bad[2 * stride + 1] = NAN;
    CHECK(ld_complex_assess(c, 4, bad.data(), stride, kept.data(), l.data(), r.data()) == LD_ERR_INVALID);
    bad[2 * stride + 1] = 0.0;
    bad[stride + 3] = 0.0;   // a zero quaternion
    CHECK(ld_complex_assess(c, 4, bad.data(), stride, kept.data(), l.data(), r.data()) == LD_ERR_INVALID);
    CHECK(ld_complex_assess(c, 4, poses.data(), len - 1, kept.data(), l.data(), r.data()) == LD_ERR_INVALID);
    CHECK(ld_complex_assess(c, 4, nullptr, stride, kept.data(), l.data(), r.data()) == LD_ERR_INVALID);
    CHECK(ld_complex_assess(nullptr, 4, poses.data(), stride, kept.data(), l.data(), r.data()) == LD_ERR_INVALID);
    CHECK(kept[0] == 0xA5A5A5A5u && kept[3] == 0xA5A5A5A5u);

    // refusals at reference time leave no reference
    for (double cutoff : {0.0, -1.0, 30.001, (double)NAN, 1e300}) {
        CHECK(ld_complex_set_reference(c, rec.c_str(), lig.c_str(), 5.0, 10.0) == LD_OK);
        CHECK(ld_complex_set_reference(c, rec.c_str(), lig.c_str(), cutoff, 10.0) == LD_ERR_INVALID);
        CHECK(ld_complex_reference_counts(c, counts) == LD_ERR_INVALID);
        CHECK(ld_complex_set_reference(c, rec.c_str(), lig.c_str(), 5.0, cutoff) == LD_ERR_INVALID);
    }
    CHECK(ld_complex_set_reference(c, rec.c_str(), lig.c_str(), 5.0, 10.0) == LD_OK);
    CHECK(ld_complex_set_reference(c, (scratch + "/no_such.pdb").c_str(), lig.c_str(), 5.0, 10.0) == LD_ERR_IO);
    CHECK(ld_complex_assess(c, 4, poses.data(), stride, kept.data(), l.data(), r.data()) == LD_ERR_INVALID);
    CHECK(ld_complex_set_reference(c, nullptr, lig.c_str(), 5.0, 10.0) == LD_ERR_INVALID);
    CHECK(ld_complex_set_reference(c, rec.c_str(), nullptr, 5.0, 10.0) == LD_ERR_INVALID);
    CHECK(ld_complex_set_reference(nullptr, rec.c_str(), lig.c_str(), 5.0, 10.0) == LD_ERR_INVALID);
    CHECK(ld_complex_set_reference(c, lig.c_str(), rec.c_str(), 5.0, 10.0) == LD_ERR_INVALID);   // the sides swapped: nothing matches
    // a reference far away in its own frame is still a reference: the centre moves with it
    CHECK(ld_complex_set_reference(c, rec.c_str(), lig.c_str(), 0.001, 0.001) == LD_ERR_INVALID);   // no native pair
    CHECK(ld_complex_reference_counts(nullptr, counts) == LD_ERR_INVALID && ld_complex_reference_counts(c, nullptr) == LD_ERR_INVALID);
    ld_complex_destroy(c);

    // hand-made complexes: the least a reference may have, and one atom less
    const std::string r3 = atom_line(1, "N", "GLY", 'A', 1, 0, 0, 0, kRest) + atom_line(2, "CA", "GLY", 'A', 1, 1.5, 0, 0, kRest) +
                           atom_line(3, "C", "GLY", 'A', 1, 1.5, 1.5, 0, kRest) + atom_line(4, "CB", "GLY", 'A', 1, 0, 1.5, 1.5, kRest);
    const std::string l1 = atom_line(1, "P", "DT", 'B', 1, 3.0, 4.0, 0, kRest) + atom_line(2, "OP1", "DT", 'B', 1, 9.0, 9.0, 9.0, kRest);
    put(scratch + "/r3.pdb", r3);
    put(scratch + "/l1.pdb", l1);
    put(scratch + "/r2.pdb", r3.substr(0, r3.find("ATOM", 100)) + atom_line(4, "CB", "GLY", 'A', 1, 0, 1.5, 1.5, kRest));   // N, CA and the CB
    put(scratch + "/l0.pdb", atom_line(2, "OP1", "DT", 'B', 1, 3.0, 4.0, 0, kRest));
    put(scratch + "/lfar.pdb", atom_line(1, "P", "DT", 'B', 1, 3.0, 4.0, 40.0, kRest));
    put(scratch + "/lvery_far.pdb", atom_line(1, "P", "DT", 'B', 1, 3.0, 4.0, 2100.0, kRest));
    ld_complex *t = ld_complex_create((scratch + "/r3.pdb").c_str(), (scratch + "/l1.pdb").c_str(), nullptr, 0, 0, nullptr, 0, 0);
    CHECK(t != nullptr);
    if (!t) return;
    const std::string R3 = scratch + "/r3.pdb", L1 = scratch + "/l1.pdb";
    CHECK(ld_complex_set_reference(t, R3.c_str(), L1.c_str(), 5.0, 10.0) == LD_OK);   // P is 3-4-5 from N, 2.92 A from C
    CHECK(ld_complex_reference_counts(t, counts) == LD_OK);
    CHECK(counts[0] == 4 && counts[1] == 2 && counts[2] == 1 && counts[3] == 3 && counts[4] == 1 && counts[5] == 4);
    CHECK(ld_complex_assess(t, 2, poses.data(), stride, kept.data(), l.data(), r.data()) == LD_OK && kept[1] == 1);
    CHECK(ld_complex_set_reference(t, R3.c_str(), L1.c_str(), 2.9, 10.0) == LD_ERR_INVALID);                         // no native pair
    CHECK(ld_complex_set_reference(t, (scratch + "/r2.pdb").c_str(), L1.c_str(), 5.0, 10.0) == LD_ERR_INVALID);      // 2 receptor fit atoms
    CHECK(ld_complex_set_reference(t, R3.c_str(), (scratch + "/l0.pdb").c_str(), 5.0, 10.0) == LD_ERR_INVALID);      // no ligand fit atom
    CHECK(ld_complex_set_reference(t, R3.c_str(), (scratch + "/lfar.pdb").c_str(), 5.0, 10.0) == LD_ERR_INVALID);    // nothing within either cutoff
    CHECK(ld_complex_set_reference(t, R3.c_str(), (scratch + "/lvery_far.pdb").c_str(), 5.0, 10.0) == LD_ERR_INVALID);
    CHECK(ld_complex_reference_counts(t, counts) == LD_ERR_INVALID);
    ld_complex_destroy(t);
}

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: assess_check <tests/golden> <scratch dir>\n");
        return 2;
    }
    numerics();
    through_the_abi(argv[1], argv[2]);
    std::printf("assess_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
