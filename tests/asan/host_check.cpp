// host_check.cpp -- TEST INFRASTRUCTURE: drives the host side of the library through its C ABI in
// the sanitizer build (tests/asan/hip_stub.cpp stands in for the HIP runtime and the kernels).
// usage: host_check <tests/golden> <scratch dir>.  Exit code 0 = every call behaved; ASan / UBSan
// report on their own (the CPU test greps for them).
#include <sys/stat.h>
#include <unistd.h>

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define CHECK_PROGRAM "host_check"
#include "check.hpp"
#include "device_memory.hpp"     // the carver is checked directly
#include "kernels/cluster.hpp"   // the analysis section sizes its inputs from the constants; every call goes through the C ABI
#include "kernels/complex_rule.hpp"   // the shared posing rule is checked directly

extern "C" size_t ld_stub_device_allocations(void);   // tests/asan/hip_stub.cpp
extern "C" size_t ld_stub_device_allocations_of(size_t bytes);
extern "C" size_t ld_stub_packed_prepare_launches(void);
extern "C" size_t ld_stub_pair_kernel_launches(void);

// A DFIRE scorer through every form of a block-major batch: plain, counting (the sequence runs twice), the single-pose call.
// Device memory is host memory in this build, so the device-pointer call takes host vectors.
// A culled route (block-major, packed) leaves the all-pairs kernel uncalled and has block counts; the all-pairs route launches it
// once a call and has none.
static void bm_batches(ld_scorer *s, size_t n, const char *want_kernel) {
    const size_t len = ld_scorer_pose_len(s);
    std::vector<double> poses(len * n, 0.0), e(n);
    for (size_t i = 0; i < n; i++) poses[len * i + 3] = 1.0;
    std::vector<uint32_t> counts(n), blocks(n);
    ld_kernel_info info;
    CHECK(ld_scorer_kernel_info(s, &info) == LD_OK && std::strcmp(info.pair_kernel_name, want_kernel) == 0);
    const bool all_pairs = std::strncmp(want_kernel, "pose_energy_pairs", 17) == 0;
    const size_t before = ld_stub_pair_kernel_launches();
    CHECK(ld_scorer_energy_batch(s, n, poses.data(), len, e.data()) == LD_OK);
    CHECK(ld_scorer_energy_batch_device(s, n, poses.data(), len, nullptr, e.data(), counts.data()) == LD_OK);
    CHECK(ld_scorer_last_block_counts(s, n, blocks.data()) == (all_pairs ? LD_ERR_UNSUPPORTED : LD_OK));
    CHECK(ld_scorer_energy_batch(s, 1, poses.data(), len, e.data()) == LD_OK);   // a smaller batch after a larger one
    CHECK(ld_stub_pair_kernel_launches() - before == (all_pairs ? 3u : 0u));
}

static int cli(std::vector<std::string> args) {
    std::vector<char *> argv;
    for (auto &a : args) argv.push_back(&a[0]);
    argv.push_back(nullptr);
    return ld_cli_main((int)args.size(), argv.data());
}

// ---- the carver every block of the analysis half is laid out with (device_memory.hpp) -------------------------------------------
struct CarvedBlock {
    int *a = nullptr;
    double *none = nullptr, *b = nullptr;
    uint8_t *odd = nullptr;
    uint64_t *last = nullptr;
};

static void carved_layout(ld::Carver &c, CarvedBlock &p) {
    p.a = c.take<int>(4);   // ends on a boundary: what follows starts at its past-the-end element
    p.none = c.take<double>(0);
    p.b = c.take<double>(3);
    p.odd = c.take<uint8_t>(5);
    p.last = c.take<uint64_t>(2);
}

static void carver() {
    CarvedBlock measured, placed;
    ld::Carver measure;
    carved_layout(measure, measured);
    // measuring hands out no address; 16 + 24 -> 40, 5 bytes at 48 -> 53, 16 bytes at 64: the extent is the last array's end
    CHECK(!measured.a && !measured.none && !measured.b && !measured.odd && !measured.last && measure.bytes() == 80);
    ld::DeviceBuffer buffer;
    ld::carve_into(buffer, [&](ld::Carver &c) { carved_layout(c, placed); });
    CHECK(buffer.bytes >= 80 && (void *)placed.a == buffer.ptr);
    ld::Carver place(buffer.ptr);
    carved_layout(place, placed);
    CHECK(place.bytes() == measure.bytes());
    for (const void *p : {(const void *)placed.a, (const void *)placed.b, (const void *)placed.odd, (const void *)placed.last})
        CHECK(p != nullptr && (uintptr_t)p % 16 == 0);
    // an array of no elements: no room, no address -- not the past-the-end element of `a`, which is where `b` starts
    CHECK(placed.none == nullptr && (void *)placed.b == (void *)(placed.a + 4));
    // both ends of every array lie inside what was reserved (the growth headroom behind it is poisoned in this build)
    placed.a[0] = placed.a[3] = 1;
    placed.b[0] = placed.b[2] = 1.0;
    placed.odd[0] = placed.odd[4] = 1;
    placed.last[0] = placed.last[1] = 1;
    ld::Carver empty;
    CHECK(empty.take<int>(0) == nullptr && empty.bytes() == 0);
    // a byte count beyond size_t is refused, in the product and in the sum, and leaves the extent as it was
    for (int what = 0; what < 2; what++) {
        ld::Carver c;
        c.take<int>(1);
        bool refused = false;
        try {
            if (what == 0) c.take<uint64_t>(SIZE_MAX / 4);
            if (what == 1) c.take<uint8_t>(SIZE_MAX - 16);
        } catch (const ld::Error &e) {
            refused = e.code() == LD_ERR_INVALID;
        }
        CHECK(refused && c.bytes() == 4);
    }
}

// ---- the posing-and-rounding rule the analysis kernels, ccs.cpp and the stubs share (kernels/complex_rule.hpp), on the host --------
static bool posed_is(const ld::ComplexDevice &m, const double *row, uint32_t atom, int bound, bool want_ok, int x, int y, int z) {
    int v[3] = {-1, -1, -1};
    return ld::posed_thousandths(m, row, atom, bound, v) == want_ok && v[0] == x && v[1] == y && v[2] == z;
}

static void complex_rule() {
    // what "%.3f" prints of each, tests/test_contacts_cpu.py's pinned values
    const double x[7] = {0.0005, -0.0004, 1.2345, -1.2346, 4.9995, -0.0, 123.4565}, want[7] = {1, 0, 1234, -1235, 5000, 0, 123457};
    for (int i = 0; i < 7; i++) CHECK(ld::thousandths(x[i]) == want[i]);
    CHECK(ld::thousandths(2.0) == 2000.0 && ld::thousandths(-12.3456) == -12346.0);

    const int B = ld::kComplexCoordBound;
    static_assert(ld::kComplexCoordBound == 1000000000 && 2ll * ld::kComplexCoordBound < (1ll << 31), "the difference of two coordinates fits an int32");
    const double identity[7] = {0, 0, 0, 1, 0, 0, 0};
    double rec[3] = {0, 0, 0}, lig[3] = {0, 0, 0};
    ld::ComplexDevice m;
    m.n_rec = 1, m.rec_xyz = rec;
    // a one-atom receptor at the bound's edge, on every axis and sign: +-1 000 000.000 A fits, one thousandth more does not
    for (int k = 0; k < 3; k++)
        for (int sign = -1; sign <= 1; sign += 2) {
            int at[3] = {0, 0, 0};
            rec[0] = rec[1] = rec[2] = 0.0;
            rec[k] = sign * 1000000.0, at[k] = sign * B;
            CHECK(posed_is(m, identity, 0, B, true, at[0], at[1], at[2]));
            rec[k] = sign * 1000000.001;
            CHECK(ld::thousandths(rec[k]) == sign * (B + 1.0) && posed_is(m, identity, 0, B, false, at[0], at[1], at[2]));   // clamped
            CHECK(posed_is(m, identity, 0, INT_MAX, true, at[0] + (k == 0) * sign, at[1] + (k == 1) * sign, at[2] + (k == 2) * sign));
            rec[k] = std::nan("");
            at[k] = B;
            CHECK(posed_is(m, identity, 0, B, false, at[0], at[1], at[2]));   // a NaN clamps to +bound; UBSan sees the conversion
            at[k] = INT_MAX;
            CHECK(posed_is(m, identity, 0, INT_MAX, false, at[0], at[1], at[2]));
        }
    rec[0] = 3.0e6, rec[1] = -3.0e6, rec[2] = 0.0;   // beyond an int32 in thousandths
    CHECK(posed_is(m, identity, 0, INT_MAX, false, INT_MAX, -INT_MAX, 0));
    // a ligand atom: identity rotation plus translation; the quaternion scaled by 2 divides by its norm^2 and gives the same integers
    m.n_lig = 1, m.lig_xyz = lig;
    for (double scale : {1.0, 2.0}) {
        double row[7] = {0, 0, 0, scale, 0, 0, 0};
        lig[0] = 1.2345, lig[1] = -1.2346, lig[2] = 4.9995;
        CHECK(posed_is(m, row, 1, B, true, 1234, -1235, 5000));
        lig[0] = 1.5, lig[1] = -2.25, lig[2] = 3.125;
        row[0] = 10.0, row[1] = 20.0, row[2] = -30.0;
        CHECK(posed_is(m, row, 1, B, true, 11500, 17750, -26875));
        const ld::P3 p = ld::pose_atom(m, row, 1);
        CHECK(p.x == 11.5 && p.y == 17.75 && p.z == -26.875);
        row[1] = 1000000.0 + 2.25, row[2] = -1000000.0 - 3.125 - 0.001;   // the ligand at the edge, and one thousandth past it
        CHECK(posed_is(m, row, 1, B, false, 11500, B, -B));
    }
}

// ---- the analysis half (complex.cpp, host/pdb_file.cpp; ld_complex_*) ---------------------------------------------------------
static std::vector<double> identity_poses(size_t n, size_t stride) {
    std::vector<double> poses(n * stride, 0.0);
    for (size_t i = 0; i < n; i++) poses[i * stride + 3] = 1.0;
    return poses;
}

static size_t count_lines(const std::string &path, size_t *longest) {
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) return 0;
    size_t lines = 0, len = 0;
    *longest = 0;
    for (int ch; (ch = std::fgetc(f)) != EOF;) {
        if (ch == '\n') {
            lines++;
            if (len > *longest) *longest = len;
            len = 0;
        } else {
            len++;
        }
    }
    std::fclose(f);
    return lines;
}

static bool refused_create(const std::string &rec, const std::string &lig, const double *rec_nm, size_t rec_len, size_t rec_anm,
                           const char *message) {
    ld_complex *c = ld_complex_create(rec.c_str(), lig.c_str(), rec_nm, rec_len, rec_anm, nullptr, 0, 0);
    if (c) ld_complex_destroy(c);
    return !c && std::strstr(ld_last_error(), message) != nullptr;
}

static void analysis(const std::string &rec1, const std::string &lig1, const std::string &scratch) {
    const double nan = std::nan("");
    ld_complex *rigid = ld_complex_create(rec1.c_str(), lig1.c_str(), nullptr, 0, 0, nullptr, 0, 0);
    CHECK(rigid != nullptr && ld_complex_pose_len(rigid) == 7);
    const size_t nr = ld_complex_num_atoms(rigid, 0), nl = ld_complex_num_atoms(rigid, 1);
    CHECK(nr == 1615 && nl == 221);
    if (rigid) ld_complex_destroy(rigid);
    std::vector<double> rec_nm(2 * nr * 3), lig_nm(3 * nl * 3);
    for (size_t i = 0; i < rec_nm.size(); i++) rec_nm[i] = 0.01 * (double)((i * 2654435761u) % 200) - 1.0;
    for (size_t i = 0; i < lig_nm.size(); i++) lig_nm[i] = 0.01 * (double)((i * 40503u) % 200) - 1.0;
    auto create = [&] { return ld_complex_create(rec1.c_str(), lig1.c_str(), rec_nm.data(), rec_nm.size(), 2, lig_nm.data(), lig_nm.size(), 3); };

    ld_complex *c = create();
    CHECK(c != nullptr);
    if (!c) return;
    const size_t len = ld_complex_pose_len(c);
    CHECK(len == 12);
    {   // coordinates (rows further apart than a pose is long), write_pdb, contacts, the residue and atom accessors
        const size_t n = 5, stride = len + 2;
        const std::vector<double> poses = identity_poses(n, stride);
        std::vector<double> xyz(n * (nr + nl) * 3);
        CHECK(ld_complex_coordinates(c, n, poses.data(), stride, xyz.data()) == LD_OK);
        CHECK(ld_complex_coordinates(c, 0, nullptr, len, nullptr) == LD_OK);
        const std::string model = scratch + "/model.pdb";
        size_t longest = 0;
        CHECK(ld_complex_write_pdb(c, poses.data(), model.c_str()) == LD_OK && count_lines(model, &longest) == nr + nl);
        CHECK(ld_complex_write_pdb(c, poses.data(), (scratch + "/no/such/dir/model.pdb").c_str()) == LD_ERR_IO);
        const size_t rres = ld_complex_num_residues(c, 0), lres = ld_complex_num_residues(c, 1);
        CHECK(rres > 0 && lres > 0 && ld_complex_num_residues(c, 2) == 0);
        std::vector<uint32_t> rec_bits(n * ((rres + 31) / 32)), lig_bits(n * ((lres + 31) / 32));
        CHECK(ld_complex_contacts(c, n, poses.data(), stride, 3.9, rec_bits.data(), lig_bits.data()) == LD_OK);
        CHECK(ld_complex_contacts(c, n, poses.data(), stride, 3.9, nullptr, nullptr) == LD_OK);
        double ms = -1.0;
        CHECK(ld_complex_last_kernel_ms(c, &ms) == LD_OK && ms == 0.0);
        char id[32];
        CHECK(ld_complex_residue_id(c, 0, 0, id, sizeof id) == LD_OK && std::strcmp(id, "E.ILE.16") == 0);
        CHECK(ld_complex_residue_id(c, 1, lres - 1, id, sizeof id) == LD_OK);
        CHECK(ld_complex_residue_id(c, 0, 0, id, std::strlen("E.ILE.16")) == LD_ERR_INVALID);   // no room for the terminator
        CHECK(ld_complex_residue_id(c, 0, rres, id, sizeof id) == LD_ERR_INVALID);
        CHECK(ld_complex_residue_id(c, 2, 0, id, sizeof id) == LD_ERR_INVALID);
        CHECK(ld_complex_residue_id(c, 0, 0, nullptr, 0) == LD_ERR_INVALID);
        std::vector<uint32_t> of(nr);
        CHECK(ld_complex_residue_of_atom(c, 0, of.data()) == LD_OK && of.back() == rres - 1);
        of.resize(nl);
        CHECK(ld_complex_residue_of_atom(c, 1, of.data()) == LD_OK && of.back() == lres - 1);
        CHECK(ld_complex_residue_of_atom(c, 2, of.data()) == LD_ERR_INVALID);
        CHECK(ld_complex_residue_of_atom(c, 0, nullptr) == LD_ERR_INVALID);
    }
    {   // clustering: swarms of kMaxGlowworms, two more than one chunk of the workspace holds, on a handle of its own (its buffers'
        // first reservations are this call's)
        ld_complex *k = create();
        CHECK(k != nullptr);
        const size_t G = ld::kMaxGlowworms, n_bb = ld_complex_num_atoms(c, 2);
        CHECK(n_bb > 0);
        const size_t chunk = ld::kClusterWorkspaceBytes / (G * n_bb * 3 * sizeof(int32_t)), n_swarms = chunk + 2;
        CHECK(chunk >= 1);
        if (k && n_bb && chunk) {
            const std::vector<double> poses = identity_poses(n_swarms * G, len);
            std::vector<double> scoring(n_swarms * G, 1.0);
            std::vector<int32_t> cluster_of(n_swarms * G), reps(n_swarms * G);
            std::vector<uint32_t> count(n_swarms);
            CHECK(ld_complex_cluster(k, n_swarms, G, poses.data(), len, scoring.data(), 4.0, cluster_of.data(), reps.data(), count.data()) == LD_OK);
            CHECK(ld_complex_cluster(k, 3, 50, poses.data(), len, scoring.data(), 4.0, cluster_of.data(), reps.data(), count.data()) == LD_OK);
            CHECK(ld_complex_cluster(k, 0, 50, nullptr, len, nullptr, 4.0, nullptr, nullptr, nullptr) == LD_OK);
        }
        if (k) ld_complex_destroy(k);
    }
    {   // every refusal of a call, by status
        std::vector<double> poses = identity_poses(4, len), scoring(4, 1.0), xyz(4 * (nr + nl) * 3);
        std::vector<int32_t> cluster_of(4), reps(4);
        std::vector<uint32_t> count(4), bits(4 * 64);
        auto cluster = [&](ld_complex *h, size_t G, const double *p, size_t stride, const double *s, double cutoff) {
            return ld_complex_cluster(h, 2, G, p, stride, s, cutoff, cluster_of.data(), reps.data(), count.data());
        };
        CHECK(cluster(c, 2, poses.data(), len, scoring.data(), 4.0) == LD_OK);
        // null arguments
        CHECK(ld_complex_pose_len(nullptr) == 0 && ld_complex_num_atoms(nullptr, 0) == 0 && ld_complex_num_residues(nullptr, 0) == 0);
        CHECK(ld_complex_coordinates(nullptr, 4, poses.data(), len, xyz.data()) == LD_ERR_INVALID);
        CHECK(ld_complex_coordinates(c, 4, poses.data(), len, nullptr) == LD_ERR_INVALID);
        CHECK(ld_complex_coordinates(c, 4, nullptr, len, xyz.data()) == LD_ERR_INVALID);
        CHECK(cluster(nullptr, 2, poses.data(), len, scoring.data(), 4.0) == LD_ERR_INVALID);
        CHECK(cluster(c, 2, nullptr, len, scoring.data(), 4.0) == LD_ERR_INVALID);
        CHECK(cluster(c, 2, poses.data(), len, nullptr, 4.0) == LD_ERR_INVALID);
        CHECK(ld_complex_cluster(c, 2, 2, poses.data(), len, scoring.data(), 4.0, nullptr, reps.data(), count.data()) == LD_ERR_INVALID);
        CHECK(ld_complex_contacts(nullptr, 4, poses.data(), len, 3.9, bits.data(), bits.data()) == LD_ERR_INVALID);
        CHECK(ld_complex_contacts(c, 4, nullptr, len, 3.9, bits.data(), bits.data()) == LD_ERR_INVALID);
        CHECK(ld_complex_write_pdb(nullptr, poses.data(), (scratch + "/x.pdb").c_str()) == LD_ERR_INVALID);
        CHECK(ld_complex_write_pdb(c, nullptr, (scratch + "/x.pdb").c_str()) == LD_ERR_INVALID);
        CHECK(ld_complex_write_pdb(c, poses.data(), nullptr) == LD_ERR_INVALID);
        double ms = 0.0;
        CHECK(ld_complex_last_kernel_ms(nullptr, &ms) == LD_ERR_INVALID && ld_complex_last_kernel_ms(c, nullptr) == LD_ERR_INVALID);
        ld_complex_destroy(nullptr);
        // poses: stride below the pose length, a NaN, a zero quaternion -- through each call that takes poses
        for (int what = 0; what < 3; what++) {
            std::vector<double> bad = poses;
            size_t stride = len;
            if (what == 0) stride = len - 1;
            if (what == 1) bad[3 * len + len - 1] = nan;   // the last mode amplitude of the last pose
            if (what == 2) bad[2 * len + 3] = 0.0;
            CHECK(ld_complex_coordinates(c, 4, bad.data(), stride, xyz.data()) == LD_ERR_INVALID);
            CHECK(cluster(c, 2, bad.data(), stride, scoring.data(), 4.0) == LD_ERR_INVALID);
            CHECK(ld_complex_contacts(c, 4, bad.data(), stride, 3.9, bits.data(), bits.data()) == LD_ERR_INVALID);
            if (what) CHECK(ld_complex_write_pdb(c, bad.data() + (what == 1 ? 3 : 2) * len, (scratch + "/x.pdb").c_str()) == LD_ERR_INVALID);
        }
        // clustering: the glowworm count, the cutoff, the scoring
        CHECK(cluster(c, 0, poses.data(), len, scoring.data(), 4.0) == LD_ERR_INVALID);
        CHECK(cluster(c, (size_t)ld::kMaxGlowworms + 1, poses.data(), len, scoring.data(), 4.0) == LD_ERR_INVALID);
        CHECK(cluster(c, 2, poses.data(), len, scoring.data(), nan) == LD_ERR_INVALID);
        for (double v : {nan, (double)INFINITY, -(double)INFINITY}) {
            std::vector<double> bad = scoring;
            bad[3] = v;
            CHECK(cluster(c, 2, poses.data(), len, bad.data(), 4.0) == LD_ERR_INVALID);
        }
        // contacts: cutoffs outside 0.001 .. 30 A, whichever way their thousandths round; the ends themselves pass
        for (double cutoff : {0.0, 0.0004, 30.001, 31.0, -1.0, nan})
            CHECK(ld_complex_contacts(c, 4, poses.data(), len, cutoff, bits.data(), bits.data()) == LD_ERR_INVALID);
        for (double cutoff : {0.001, 30.0})
            CHECK(ld_complex_contacts(c, 4, poses.data(), len, cutoff, bits.data(), bits.data()) == LD_OK);
    }
    ld_complex_destroy(c);

    {   // files and modes a handle is refused for
        const std::string bad = scratch + "/bad_complex.pdb", good = atom_line(1, " CA", "ALA", 'A', 1, 1.0, 2.0, 3.0);
        CHECK(good.size() == 54);
        CHECK(refused_create(scratch + "/missing.pdb", lig1, nullptr, 0, 0, "cannot open PDB file"));
        CHECK(refused_create(rec1, scratch + "/missing.pdb", nullptr, 0, 0, "cannot open PDB file"));
        put(bad, "");
        CHECK(refused_create(bad, lig1, nullptr, 0, 0, "no ATOM/HETATM records"));
        put(bad, "REMARK nothing else\nEND\n");
        CHECK(refused_create(bad, lig1, nullptr, 0, 0, "no ATOM/HETATM records"));
        put(bad, good + "\n" + good.substr(0, 53) + "\n");
        CHECK(refused_create(bad, lig1, nullptr, 0, 0, "shorter than 54 columns"));
        put(bad, "ATOM\n");
        CHECK(refused_create(rec1, bad, nullptr, 0, 0, "no ATOM/HETATM records"));   // "ATOM" alone is no record
        put(bad, "HETATM\n");
        CHECK(refused_create(rec1, bad, nullptr, 0, 0, "shorter than 54 columns"));
        put(bad, good.substr(0, 38) + "   abc  " + good.substr(46) + "\n");
        CHECK(refused_create(bad, lig1, nullptr, 0, 0, "unreadable coordinate"));
        CHECK(refused_create(rec1, lig1, rec_nm.data(), rec_nm.size() - 1, 2, "mode values"));
        CHECK(refused_create(rec1, lig1, rec_nm.data(), rec_nm.size(), 3, "mode values"));
        CHECK(refused_create(rec1, lig1, nullptr, rec_nm.size(), 2, "mode values"));
        ld_complex *none = ld_complex_create(nullptr, lig1.c_str(), nullptr, 0, 0, nullptr, 0, 0);
        CHECK(none == nullptr);
    }
    {   // "\r\n" line ends, records of exactly 54 columns, records that are not atoms: one line out per record in, no '\r'
        std::string text = "REMARK a file from elsewhere\r\n";
        for (int a = 0; a < 7; a++) text += atom_line(a + 1, a % 2 ? " CA" : " N", "GLY", 'A', 1 + a / 2, a, 2.0 * a, -a) + "\r\n";
        text += "TER\r\nEND\r\n";
        const std::string crlf = scratch + "/crlf.pdb", model = scratch + "/crlf_model.pdb";
        put(crlf, text);
        ld_complex *w = ld_complex_create(crlf.c_str(), crlf.c_str(), nullptr, 0, 0, nullptr, 0, 0);
        CHECK(w != nullptr && ld_complex_num_atoms(w, 0) == 7 && ld_complex_num_atoms(w, 2) == 6 && ld_complex_num_residues(w, 1) == 4);
        if (w) {
            const std::vector<double> pose = identity_poses(1, 7);
            size_t longest = 0;
            CHECK(ld_complex_write_pdb(w, pose.data(), model.c_str()) == LD_OK);
            CHECK(count_lines(model, &longest) == 14 && longest == 54);
            ld_complex_destroy(w);
        }
    }
    {   // residue boxes that do not fit kMaxBoxLdsBytes (24 bytes a box: one-atom residues, more than 1706 of them), so that a
        // workspace slot also holds the boxes; more poses than kContactSlots, so that slots are reused
        const int n_rec = 1800, n_lig = 12;
        CHECK((size_t)(n_rec + n_lig + (n_lig + ld::kResGroup - 1) / ld::kResGroup) * 24 > ld::kMaxBoxLdsBytes);
        std::string rec, lig;
        for (int a = 0; a < n_rec; a++) rec += atom_line(a + 1, " CA", "ALA", 'A', a + 1, a % 30, (a / 30) % 30, a / 900) + "\n";
        for (int a = 0; a < n_lig; a++) lig += atom_line(a + 1, " P", "  A", 'A', a + 1, 40.0 + a, 0.0, 0.0) + "\n";
        put(scratch + "/wide_rec.pdb", rec);
        put(scratch + "/wide_lig.pdb", lig);
        ld_complex *w = ld_complex_create((scratch + "/wide_rec.pdb").c_str(), (scratch + "/wide_lig.pdb").c_str(), nullptr, 0, 0, nullptr, 0, 0);
        CHECK(w != nullptr && ld_complex_num_residues(w, 0) == (size_t)n_rec && ld_complex_num_residues(w, 1) == (size_t)n_lig);
        if (w) {
            const size_t n = ld::kContactSlots + 6;
            const std::vector<double> poses = identity_poses(n, 7);
            std::vector<uint32_t> rec_bits(n * ((n_rec + 31) / 32)), lig_bits(n * ((n_lig + 31) / 32));
            CHECK(ld_complex_contacts(w, n, poses.data(), 7, 5.0, rec_bits.data(), lig_bits.data()) == LD_OK);
            CHECK(ld_complex_contacts(w, 2, poses.data(), 7, 5.0, rec_bits.data(), lig_bits.data()) == LD_OK);   // fewer poses than slots
            ld_complex_destroy(w);
        }
    }
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const std::string gold = argv[1], scratch = argv[2];
    CHECK(ld_init(0) == LD_OK);
    CHECK(ld_device_count() == 1);

    // ---- host-only helpers ---------------------------------------------------------------------
    std::vector<uint8_t> lut(901);
    std::vector<double> steps(21);
    double iface = 0;
    CHECK(ld_dfire_bin_lut(lut.data(), steps.data(), &iface) == LD_OK);
    for (int cells = 1; cells <= 2; cells++) {
        std::vector<uint32_t> words(1028 * cells);
        double eps = 0;
        CHECK(ld_dfire_packed_lut(cells, 256.0, words.data(), &eps) == LD_OK && eps > 0);
    }
    CHECK(ld_dfire_packed_lut(3, 256.0, nullptr, nullptr) != LD_OK);
    uint32_t key[8];
    ld_stdrng_key(324324, key);

    // ---- model builders (src/dfire.rs:115-190, src/dna.rs:249-364, src/pydock.rs) ----------------
    const std::string rec1 = gold + "/1ppe/lightdock_1ppe_e.pdb", lig1 = gold + "/1ppe/lightdock_1ppe_i.pdb";
    const char *active[] = {"E.ILE.16", "E.XXX.999"};
    for (int method = 0; method < 3; method++) {
        const std::string pdb = method == 0 ? rec1 : gold + "/unit/1azp/1azp_ligand.pdb";
        ld_model *m = ld_model_from_pdb(method, pdb.c_str(), active, 2, nullptr, 0, nullptr, 0, 0);
        CHECK(m != nullptr);
        if (!m) continue;
        ld_molecule mol;
        CHECK(ld_model_view(m, &mol) == LD_OK && mol.n_atoms > 0);
        if (method == 0) {
            std::vector<uint32_t> order((mol.n_atoms + 63) / 64 * 64), perm(169);
            CHECK(ld_spatial_tile_order(mol.coordinates, mol.n_atoms, order.data()) == order.size());
            CHECK(ld_dfire_tile_layout(mol.coordinates, mol.dfire_types, mol.n_atoms, order.data(), perm.data()) == order.size());
        }
        ld_model_destroy(m);
    }
    CHECK(ld_model_from_pdb(0, (scratch + "/missing.pdb").c_str(), nullptr, 0, nullptr, 0, nullptr, 0, 0) == nullptr);
    {   // unsupported residue / atom, short line, empty file
        const std::string bad = scratch + "/bad.pdb";
        const char *texts[] = {"ATOM      1  N   XXX A   1      11.104  13.207   2.100  1.00  0.00           N\n",
                               "ATOM      1  H1  ALA A   1      11.104  13.207   2.100  1.00  0.00           H\n",
                               "ATOM      1  N   ALA A   1      11.1\n", ""};
        for (const char *t : texts) {
            FILE *f = std::fopen(bad.c_str(), "w");
            std::fputs(t, f);
            std::fclose(f);
            ld_model *m = ld_model_from_pdb(0, bad.c_str(), nullptr, 0, nullptr, 0, nullptr, 0, 0);
            if (m) ld_model_destroy(m);
        }
    }

    // ---- DCparams (src/dfire.rs:236-257) -----------------------------------------------------------
    std::vector<double> table(LD_DFIRE_TABLE_LEN);
    mkdir((scratch + "/data").c_str(), 0755);
    const std::string dc = scratch + "/data/DCparams";
    {
        FILE *f = std::fopen(dc.c_str(), "w");
        for (int i = 0; i < 1000; i++) std::fprintf(f, "%.9f\n", 0.001 * i);
        std::fclose(f);
        CHECK(ld_load_dcparams(dc.c_str(), table.data()) != LD_OK);          // too short
        f = std::fopen(dc.c_str(), "w");
        for (size_t i = 0; i < LD_DFIRE_TABLE_LEN + 5; i++) std::fprintf(f, "%.9f\n", (double)((i * 2654435761u) % 4000) / 1000.0 - 2.0);
        std::fclose(f);
        CHECK(ld_load_dcparams(dc.c_str(), table.data()) == LD_OK);
        CHECK(ld_load_dcparams((scratch + "/nope").c_str(), table.data()) != LD_OK);
    }

    // ---- scorer + GSO bookkeeping (kernels stubbed) ---------------------------------------------
    ld_scorer *s = ld_scorer_create_from_pdb(LD_METHOD_DFIRE, rec1.c_str(), lig1.c_str(), active, 1, nullptr, 0, nullptr, 0, 0,
                                             nullptr, 0, nullptr, 0, nullptr, 0, 0, 0, table.data());
    CHECK(s != nullptr);
    if (s) {
        CHECK(ld_scorer_pose_len(s) == 7 && ld_scorer_num_atoms(s, 0) == 1615 && ld_scorer_num_atoms(s, 1) == 221);
        std::vector<double> poses(7 * 300, 0.0), e(300);
        for (int i = 0; i < 300; i++) poses[7 * i + 3] = 1.0;
        CHECK(ld_scorer_energy_batch(s, 300, poses.data(), 7, e.data()) == LD_OK);
        CHECK(ld_scorer_energy_batch(s, 3, poses.data(), 5, e.data()) != LD_OK);   // stride shorter than a pose row
        double one = 1.0;
        const double t0[3] = {0, 0, 0}, q0[4] = {1, 0, 0, 0};
        CHECK(ld_scorer_energy(s, t0, q0, nullptr, nullptr, &one) == LD_OK);
        ld_kernel_info info;
        CHECK(ld_scorer_kernel_info(s, &info) == LD_OK);
        bm_batches(s, 300, "dfire_bm_pairs");
        std::vector<double> swarms(7 * 2 * 50, 0.0);
        for (int i = 0; i < 100; i++) swarms[7 * i + 3] = 1.0;
        ld_gso *g = ld_gso_create(s, 2, 50, swarms.data(), nullptr);
        CHECK(g != nullptr);
        if (g) {
            CHECK(ld_gso_run(g, 13) == LD_OK && ld_gso_steps_done(g) == 13);
            (void)ld_gso_num_evals(g);
            const std::string d0 = scratch + "/swarm_a", d1 = scratch + "/swarm_b";
            mkdir(d0.c_str(), 0755);
            mkdir(d1.c_str(), 0755);
            CHECK(ld_gso_save(g, 1, 13, d0.c_str()) == LD_OK);
            const size_t ids[2] = {0, 1};
            const char *dirs[2] = {d0.c_str(), d1.c_str()};
            CHECK(ld_gso_save_many(g, 2, ids, dirs, 13) == LD_OK);
            const size_t bad_ids[1] = {7};
            CHECK(ld_gso_save_many(g, 1, bad_ids, dirs, 13) != LD_OK);
            CHECK(ld_gso_save(g, 0, 13, (scratch + "/no/such/dir").c_str()) != LD_OK);
            std::vector<double> rp(7 * 50), luc(50), vis(50), sco(50);
            std::vector<int32_t> nn(50), mv(50), tg(50);
            CHECK(ld_gso_read(g, 1, rp.data(), luc.data(), vis.data(), sco.data(), nn.data(), mv.data(), tg.data()) == LD_OK);
            CHECK(ld_gso_read(g, 2, rp.data(), luc.data(), vis.data(), sco.data(), nn.data(), mv.data(), tg.data()) != LD_OK);
            ld_gso_destroy(g);
        }
        CHECK(ld_gso_create(s, 0, 50, swarms.data(), nullptr) == nullptr);
        ld_scorer_destroy(s);
    }
    // ---- the block-major path's object (scorer.hpp, BlockMajorPath): construction, reserve, run, destruction ----------------
    auto dfire = [&](const double *rec_nm, const double *lig_nm, size_t num_anm, const double *potential) {
        return ld_scorer_create_from_pdb(LD_METHOD_DFIRE, rec1.c_str(), lig1.c_str(), active, 1, nullptr, 0, rec_nm, rec_nm ? 1615 * 3 * num_anm : 0,
                                         num_anm, nullptr, 0, nullptr, 0, lig_nm, lig_nm ? 221 * 3 * num_anm : 0, num_anm, rec_nm ? 1 : 0, potential);
    };
    // a batch larger than a forced small pass: two workspace sets on two streams, then (LIGHTDOCK_BM_LANES=1) one set, pass after pass;
    // 300 poses = 18 passes of 16 and one of 12
    setenv("LIGHTDOCK_BM_CHUNK", "16", 1);
    for (int lanes = 2; lanes >= 1; lanes--) {
        if (lanes == 1) setenv("LIGHTDOCK_BM_LANES", "1", 1);
        ld_scorer *c = dfire(nullptr, nullptr, 0, table.data());
        CHECK(c != nullptr);
        if (!c) continue;
        bm_batches(c, 300, "dfire_bm_pairs");
        if (lanes == 2) {   // the per-wave debug words (read per call)
            const std::string dbg = scratch + "/bm_debug.txt";
            setenv("LIGHTDOCK_BM_DEBUG", dbg.c_str(), 1);
            bm_batches(c, 40, "dfire_bm_pairs");
            unsetenv("LIGHTDOCK_BM_DEBUG");
            CHECK(access(dbg.c_str(), R_OK) == 0);
        }
        ld_scorer_destroy(c);
    }
    unsetenv("LIGHTDOCK_BM_LANES");
    {   // molecules that flex: the ANM form (amplitudes by row, the flexed receptor's boxes), passes of 16 and the default pass
        std::vector<double> rec_nm(1615 * 3 * 10), lig_nm(221 * 3 * 10);
        for (size_t i = 0; i < rec_nm.size(); i++) rec_nm[i] = 0.01 * (double)((i * 2654435761u) % 200) - 1.0;
        for (size_t i = 0; i < lig_nm.size(); i++) lig_nm[i] = 0.01 * (double)((i * 40503u) % 200) - 1.0;
        for (int pass = 0; pass < 2; pass++) {
            if (pass == 1) unsetenv("LIGHTDOCK_BM_CHUNK");
            ld_scorer *a = dfire(rec_nm.data(), lig_nm.data(), 10, table.data());
            CHECK(a != nullptr);
            if (!a) continue;
            CHECK(ld_scorer_pose_len(a) == 27);
            bm_batches(a, 70, "dfire_bm_pairs");
            ld_scorer_destroy(a);
        }
    }
    {   // a complex the path declines (a table value beyond the fixed-point sums' limit): the pose-major kernel, and nothing
        // allocated for the block-major path -- construction allocates what a scorer that never asks for the path does
        std::vector<double> big(table);
        big[12345] = 2000.0;
        size_t before = ld_stub_device_allocations();
        ld_scorer *d = dfire(nullptr, nullptr, 0, big.data());
        const size_t declined = ld_stub_device_allocations() - before;
        CHECK(d != nullptr);
        if (d) {
            uint32_t quiet = 1;
            CHECK(ld_scorer_bm_quiet_subtiles(d, &quiet) == LD_OK && quiet == 0);
            bm_batches(d, 70, "dfire_packed_pairs");
            ld_scorer_destroy(d);
        }
        setenv("LIGHTDOCK_DFIRE_KERNEL", "packed", 1);
        before = ld_stub_device_allocations();
        d = dfire(nullptr, nullptr, 0, big.data());
        CHECK(d != nullptr && ld_stub_device_allocations() - before == declined);
        if (d) ld_scorer_destroy(d);
        unsetenv("LIGHTDOCK_DFIRE_KERNEL");
    }
    {   // and the mirror: a rigid scorer builds the receptor image of the route it runs, once -- nothing of the packed route under a
        // block-major scorer, nothing of either culled route under the all-pairs kernel
        const char *kernels[3] = {nullptr, "packed", "allpairs"};
        const char *names[3] = {"dfire_bm_pairs", "dfire_packed_pairs", "pose_energy_pairs<0"};
        const size_t want[3] = {1, 1, 0};
        // the potential in the reference's layout (LD_DFIRE_TABLE_LEN doubles; the culled routes' patch table has another size) is
        // the all-pairs route's alone
        const size_t table_bytes = LD_DFIRE_TABLE_LEN * sizeof(double), want_tables[3] = {0, 0, 1};
        for (int k = 0; k < 3; k++) {
            if (kernels[k]) setenv("LIGHTDOCK_DFIRE_KERNEL", kernels[k], 1);
            const size_t before = ld_stub_packed_prepare_launches(), tables_before = ld_stub_device_allocations_of(table_bytes);
            ld_scorer *c = dfire(nullptr, nullptr, 0, table.data());
            CHECK(c != nullptr && ld_stub_packed_prepare_launches() - before == want[k]);
            CHECK(ld_stub_device_allocations_of(table_bytes) - tables_before == want_tables[k]);
            ld_kernel_info info;
            CHECK(c && ld_scorer_kernel_info(c, &info) == LD_OK && std::strcmp(info.pair_kernel_name, names[k]) == 0);
            if (c) bm_batches(c, 70, names[k]);
            if (c) ld_scorer_destroy(c);
            unsetenv("LIGHTDOCK_DFIRE_KERNEL");
        }
    }
    {   // a DNA scorer (restraints on both sides): the all-pairs route without a DFIRE table; LIGHTDOCK_CHUNK_ATOMS: more
        // receptor chunks, i.e. partials a pose, than the default
        const std::string base = gold + "/unit/1azp/";
        const char *rec_active[] = {"A.MET.1"}, *lig_active[] = {"B.DG.1"};
        for (int chunked = 0; chunked < 2; chunked++) {
            if (chunked) setenv("LIGHTDOCK_CHUNK_ATOMS", "64", 1);
            const size_t tables_before = ld_stub_device_allocations_of(LD_DFIRE_TABLE_LEN * sizeof(double));
            ld_scorer *c = ld_scorer_create_from_pdb(LD_METHOD_DNA, (base + "1azp_receptor.pdb").c_str(), (base + "1azp_ligand.pdb").c_str(), rec_active, 1,
                                                     nullptr, 0, nullptr, 0, 0, lig_active, 1, nullptr, 0, nullptr, 0, 0, 0, nullptr);
            CHECK(c != nullptr && ld_stub_device_allocations_of(LD_DFIRE_TABLE_LEN * sizeof(double)) == tables_before);
            if (c) bm_batches(c, 70, "pose_energy_pairs<1");
            if (c) ld_scorer_destroy(c);
        }
        unsetenv("LIGHTDOCK_CHUNK_ATOMS");
    }
    CHECK(ld_scorer_create_from_pdb(7, rec1.c_str(), lig1.c_str(), nullptr, 0, nullptr, 0, nullptr, 0, 0, nullptr, 0, nullptr, 0,
                                    nullptr, 0, 0, 0, table.data()) == nullptr);

    carver();
    complex_rule();
    analysis(rec1, lig1, scratch);

    // ---- the CLI (src/bin/lightdock-rust.rs:77-333): usage errors return 0, panics 101 ---------------
    CHECK(chdir(scratch.c_str()) == 0);
    CHECK(cli({"lightdock-hip"}) == 0);
    (void)cli({"lightdock-hip", gold + "/1ppe/setup.json", gold + "/1ppe/initial_positions_0.dat", "abc", "dfire"});   // exit codes: tests/test_host_cpu.py
    CHECK(cli({"lightdock-hip", gold + "/1ppe/setup.json", gold + "/1ppe/initial_positions_0.dat", "2", "nomethod"}) == 0);
    (void)cli({"lightdock-hip", scratch + "/nosetup.json", gold + "/1ppe/initial_positions_0.dat", "2", "dfire"});
    CHECK(cli({"lightdock-hip", gold + "/1ppe/setup.json", gold + "/1ppe/initial_positions_0.dat", "2", "dfire"}) == 0);   // data/DCparams from above
    // DNA + ANM: rec_nm.npy / lig_nm.npy from the CWD
    for (const char *f : {"rec_nm.npy", "lig_nm.npy"}) {
        std::string cmd = "cp " + gold + "/1azp/" + f + " " + scratch + "/";
        CHECK(std::system(cmd.c_str()) == 0);
    }
    CHECK(cli({"lightdock-hip", gold + "/1azp/setup.json", gold + "/1azp/initial_positions_0.dat", "2", "dna"}) == 0);
    {   // a truncated .npy must be refused, not read past its end
        FILE *f = std::fopen((scratch + "/rec_nm.npy").c_str(), "r+");
        if (f) { CHECK(ftruncate(fileno(f), 200) == 0); std::fclose(f); }
        CHECK(cli({"lightdock-hip", gold + "/1azp/setup.json", gold + "/1azp/initial_positions_0.dat", "2", "dna"}) != 0);
    }
    std::fprintf(stderr, "host_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
