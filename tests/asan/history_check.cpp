// history_check.cpp -- driver of the sanitizer build across the entries of one ld_complex* handle (`make asan-history`;
// tests/test_asan_history.py): all sixteen device entries through the C ABI against tests/asan/hip_stub*.cpp (device memory =
// host memory; the launches do their kernels' work in plain C++), in the histories of tests/handle_history.py at the driver's
// own small sizes.  On a handle with receptor modes and on one without: every large DECOY once; then, for every entry X and
// every entry Y, decoy(X) and the small probe(Y); a decoy refused for a far pose, a short stride, a NaN or a zero quaternion
// and every probe after it (the far pose is
// found by the launches that pose: the stubs of cluster, contacts and assess do not); a refused reference; probes, decoys, probes on a fresh handle; the two handles turn by turn on
// one ld_density.  device_memory.hpp's reserve_exact() closes every shared block beyond what the call at hand carved, so an
// offset a probe takes beyond its own extent is reported although a decoy left the block larger.  What ASan and UBSan report
// is the point; that every probe's outputs are the bytes the same probe gives on a fresh handle is a guard (the stubs are
// not the kernels: tests/test_gpu_handle_history.py holds the kernels to their references).
//   usage: history_check <scratch dir>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#define CHECK_PROGRAM "history_check"
#include "check.hpp"

typedef std::vector<unsigned char> Bytes;

enum Entry { COORDINATES, CLUSTER, CLUSTER_RANKED, CONTACTS, PAIR_CONTACTS, CLUSTER_FCC, SASA, CCS, CROSSLINKS, DISTANCE_HISTOGRAM, SAXS,
             DENSITY_FIT, SIMULATE_DENSITY, ASSESS, SET_REFERENCE, WRITE_PDB, N_ENTRIES };
static const char *const NAMES[N_ENTRIES] = {"coordinates", "cluster", "cluster_ranked", "contacts", "pair_contacts", "cluster_fcc", "sasa", "ccs",
                                             "crosslinks", "distance_histogram", "saxs", "density_fit", "simulate_density", "assess",
                                             "set_reference", "write_pdb"};
enum How { GOOD, FAR, STRIDE, NOT_A_NUMBER, ZERO_QUATERNION };

static const int N_REC_RES = 6, N_LIG_RES = 3, PER_RES = 5;                 // N, CA, C, O, HA; and one MMB bead a side
static const int N_REC = N_REC_RES * PER_RES + 1, N_LIG = N_LIG_RES * PER_RES + 1;
static const size_t PROBE_N = 2, DECOY_N = 16;

struct World {
    std::string scratch, rec, lig, ref_a[2], ref_b[2];
    std::vector<double> rec_modes, lig_modes;
    ld_density *map[2];
};
static World W;

// A generator of its own: the same numbers on every platform.
struct Lcg {
    uint64_t s;
    explicit Lcg(uint64_t seed) : s(seed * 2862933555777941757ull + 3037000493ull) {}
    double next() {   // (-1, 1)
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (double)((s >> 11) & ((1ull << 52) - 1)) / (double)(1ull << 51) - 1.0;
    }
};

static std::string rest(const char *element) {
    char buf[64];
    std::snprintf(buf, sizeof buf, "  1.00  0.00          %2s  \n", element);
    return buf;
}

// One side's file; `skip` leaves a residue out, `shift` moves every atom along x (a reference of another shape and place).
static std::string side_text(bool ligand, int skip, double shift) {
    static const char *const names[PER_RES] = {"N", "CA", "C", "O", "HA"};
    static const char *const elements[PER_RES] = {"N", "C", "C", "O", "H"};
    static const double at[PER_RES][3] = {{0, 0, 0}, {1.4, 0.3, 0}, {2.1, 1.2, 0.5}, {2.4, 2.2, -0.4}, {1.6, -0.6, 0.7}};
    std::string text;
    int serial = 1;
    const int n_res = ligand ? N_LIG_RES : N_REC_RES;
    for (int r = 0; r < n_res; r++)
        for (int a = 0; a < PER_RES; a++, serial++) {
            if (r == skip) continue;
            const double x = 4.0 * r + (ligand ? 1.0 : 0.0) + at[a][0] + shift, y = (ligand ? 4.2 : 0.0) + at[a][1], z = (ligand ? 1.0 : 0.0) + at[a][2];
            text += atom_line(serial, names[a], "SER", ligand ? 'B' : 'A', r + 1, x, y, z, rest(elements[a]).c_str());
        }
    text += atom_line(serial, "BJ", "MMB", ligand ? 'B' : 'A', n_res + 1, ligand ? 6.0 : 10.0, ligand ? 9.0 : -5.0, 3.0 + shift, rest("C").c_str());
    return text;
}

static ld_complex *make(bool flex) {
    return ld_complex_create(W.rec.c_str(), W.lig.c_str(), flex ? W.rec_modes.data() : nullptr, flex ? W.rec_modes.size() : 0, flex ? 2 : 0,
                             W.lig_modes.data(), W.lig_modes.size(), 2);
}

// n rows of `stride` doubles: a small translation, a quaternion near a random one, amplitudes below 1; what lies beyond the pose
// length is large and must never be read.  `twins`: row i + 1 the copy of row i, for even i, but for a hundredth of an A.
static std::vector<double> poses_of(int entry, int kind, size_t n, size_t len, size_t stride, bool twins) {
    Lcg g((uint64_t)entry * 7 + (uint64_t)kind * 131 + len);
    std::vector<double> p(n * stride);
    for (size_t i = 0; i < n; i++) {
        double *row = &p[i * stride];
        if (twins && i % 2 == 1) {
            std::copy(row - stride, row, row);
            row[0] += 0.01;
            continue;
        }
        for (size_t k = 0; k < stride; k++) row[k] = k < 3 ? 1.5 * g.next() : k < 7 ? g.next() : k < len ? 0.8 * g.next() : 1e5 * g.next();
        row[3] += row[3] < 0 ? -0.5 : 0.5;   // never a zero quaternion
    }
    return p;
}

template <typename T>
static void append(Bytes &out, const std::vector<T> &v) {
    const unsigned char *p = reinterpret_cast<const unsigned char *>(v.data());
    out.insert(out.end(), p, p + v.size() * sizeof(T));
}

// One configured call: entry, kind (0 the probe, 1 the decoy), how its last pose is spoilt.  Returns the status; `out` takes
// every output's bytes.
static int run(ld_complex *c, int entry, int kind, int how, Bytes &out) {
    out.clear();
    const size_t len = ld_complex_pose_len(c);
    const bool decoy = kind >= 1;   // 2: the one call of the soak whose size the sweep cannot afford (crosslinks alone)
    size_t n = decoy ? DECOY_N : PROBE_N, stride = decoy ? len + 3 : len;
    if (entry == CROSSLINKS) n = kind == 1 ? 2 : 1;
    if (entry == CCS && decoy) n = 8;
    if (entry == WRITE_PDB) n = 1, stride = len;
    const bool clustering = entry == CLUSTER || entry == CLUSTER_RANKED || entry == CLUSTER_FCC;
    std::vector<double> poses = poses_of(entry, kind, n, len, stride, clustering);
    double *last = &poses[(n - 1) * stride];
    if (how == FAR) last[0] = entry == CLUSTER || entry == CLUSTER_RANKED ? 2.2e6 : 1.1e6;
    if (how == NOT_A_NUMBER) last[5] = NAN;
    if (how == ZERO_QUATERNION) last[3] = last[4] = last[5] = last[6] = 0.0;
    if (how == STRIDE) stride = len - 1;   // refused before a row is read
    std::vector<double> scoring(n);
    Lcg g((uint64_t)entry * 17 + (uint64_t)kind);
    for (double &s : scoring) s = 10.0 * g.next();
    const size_t n_atoms = (size_t)(N_REC + N_LIG);
    const double *P = poses.data();
    int status = LD_ERR_INVALID;
    switch (entry) {
    case COORDINATES: {
        std::vector<double> xyz(n * n_atoms * 3, -1.0);
        status = ld_complex_coordinates(c, n, P, stride, xyz.data());
        append(out, xyz);
        break;
    }
    case CLUSTER: {
        const size_t swarms = decoy ? 4 : 1, G = n / swarms;
        std::vector<int32_t> of(n, -7), reps(n, -7);
        std::vector<uint32_t> k(swarms, 77);
        status = ld_complex_cluster(c, swarms, G, P, stride, scoring.data(), decoy ? 2.5 : 1.0, of.data(), reps.data(), k.data());
        append(out, of), append(out, reps), append(out, k);
        break;
    }
    case CLUSTER_RANKED: {
        std::vector<int32_t> of(n, -7), reps(n, -7);
        std::vector<uint32_t> k(1, 77);
        status = ld_complex_cluster_ranked(c, n, P, stride, scoring.data(), decoy ? 2.5 : 1.0, decoy ? 1 : 0, of.data(), reps.data(), k.data());
        append(out, of), append(out, reps), append(out, k);
        break;
    }
    case CONTACTS: {
        std::vector<uint32_t> rec(n, 77), lig(n, 77);   // one word a side
        status = ld_complex_contacts(c, n, P, stride, decoy ? 7.5 : 4.0, rec.data(), decoy ? lig.data() : nullptr);
        append(out, rec), append(out, lig);
        break;
    }
    case PAIR_CONTACTS: {
        std::vector<uint32_t> offsets(n + 1, 77), keys(n * (N_REC_RES + 1) * (N_LIG_RES + 1), 77);
        size_t total = 0;
        status = ld_complex_pair_contacts(c, n, P, stride, decoy ? 6.5 : 5.0, offsets.data(), keys.data(), keys.size(), &total);
        if (status == LD_OK) keys.resize(total);
        append(out, offsets), append(out, keys);
        break;
    }
    case CLUSTER_FCC: {
        std::vector<int32_t> of(n, -7), centres(n, -7);
        std::vector<uint32_t> k(1, 77), sizes(n, 77);
        std::vector<uint64_t> consensus(n, 77);
        status = ld_complex_cluster_fcc(c, n, P, stride, scoring.data(), decoy ? 6.0 : 5.0, decoy ? 0.4 : 0.6, decoy ? 2 : 1, of.data(), centres.data(),
                                        k.data(), decoy ? sizes.data() : nullptr, decoy ? consensus.data() : nullptr);
        append(out, of), append(out, centres), append(out, k), append(out, sizes), append(out, consensus);
        break;
    }
    case SASA: {
        std::vector<uint64_t> sums(n * 4, 77);
        std::vector<uint8_t> free_counts(n * n_atoms, 77), bound(n * n_atoms, 77);
        status = ld_complex_sasa(c, n, P, stride, decoy ? 1.0 : 1.4, sums.data(), decoy ? free_counts.data() : nullptr, decoy ? bound.data() : nullptr);
        append(out, sums), append(out, free_counts), append(out, bound);
        break;
    }
    case CCS: {
        std::vector<uint32_t> counts(n * LD_CCS_VIEWS, 77);
        std::vector<uint64_t> sums(n, 77);
        // the rigid form's bitmaps (what == 2, no receptor modes) laid out for a finer cell by the decoy; another selection where the receptor flexes
        status = ld_complex_ccs(c, n, P, stride, decoy && len == 11 ? 1 : 2, decoy ? 1.5 : 1.0, decoy ? 0.5 : 1.0, decoy ? counts.data() : nullptr, sums.data());
        append(out, counts), append(out, sums);
        break;
    }
    case CROSSLINKS: {
        // anchors: receptor O of residues 1 and 4, a receptor N, ligand O of residues 0 and 2, a ligand CA
        const uint32_t a = 1 * PER_RES + 3, b = 4 * PER_RES + 3, e = 5 * PER_RES, x = N_REC + 3, y = N_REC + 2 * PER_RES + 3, z = N_REC + PER_RES + 1;
        const std::vector<uint32_t> links = decoy ? std::vector<uint32_t>{x, a, x, b, x, e, x, y, x, z} : std::vector<uint32_t>{a, x, a, y, b, z, b, e};
        const size_t L = links.size() / 2;
        std::vector<uint64_t> straight2(n * L, 77);
        std::vector<uint32_t> path(n * L, 77);
        // the soak's one large call keeps the bits of its box (77^3 nodes) in the slot; the decoy's box (43^3) and the probe's
        // (15^3) keep theirs in LDS: the stub walks every node, and the sweep runs the decoy before every probe
        status = ld_complex_crosslinks(c, n, P, stride, L, links.data(), decoy ? 0.3 : 0.0, decoy ? 0.5 : 1.0, decoy ? 2.5 : 3.0,
                                       kind == 2 ? 18.5 : decoy ? 10.0 : 6.0, straight2.data(), path.data());
        append(out, straight2), append(out, path);
        break;
    }
    case DISTANCE_HISTOGRAM: {
        const size_t bins = decoy ? 1024 : 128;
        std::vector<uint32_t> counts(n * 21 * bins, 77);
        status = ld_complex_distance_histogram(c, n, P, stride, decoy ? 250 : 500, bins, counts.data());
        append(out, counts);
        break;
    }
    case SAXS: {
        const size_t bins = decoy ? 512 : 128;
        const std::vector<double> q = decoy ? std::vector<double>{0.01, 0.1, 0.2, 0.3, 0.45, 0.6, 0.9} : std::vector<double>{0.0, 0.05, 0.5};
        std::vector<double> intensity(n * q.size(), -1.0);
        std::vector<uint32_t> counts(n * 21 * bins, 77);
        status = ld_complex_saxs(c, n, P, stride, decoy ? 300 : 500, bins, q.data(), q.size(), intensity.data(), decoy ? counts.data() : nullptr);
        append(out, intensity), append(out, counts);
        break;
    }
    case DENSITY_FIT: {
        std::vector<ld_density_sums> sums(n);
        std::memset(sums.data(), 0x4D, n * sizeof(ld_density_sums));
        status = ld_complex_density_fit(c, W.map[kind], n, P, stride, decoy ? 3000 : 2000, sums.data());
        append(out, sums);
        break;
    }
    case SIMULATE_DENSITY: {
        uint64_t N = 0;
        CHECK(ld_density_info(W.map[kind], &N, nullptr, nullptr, nullptr) == LD_OK);
        std::vector<uint32_t> grid(n * N, 77);
        status = ld_complex_simulate_density(c, W.map[kind], n, P, stride, decoy ? 3000 : 2000, grid.data());
        append(out, grid);
        break;
    }
    case ASSESS:
    case SET_REFERENCE: {
        const std::string *ref = decoy ? W.ref_b : W.ref_a;
        status = ld_complex_set_reference(c, ref[0].c_str(), ref[1].c_str(), decoy ? 6.0 : 5.0, decoy ? 12.0 : 10.0);
        if (status != LD_OK) break;
        if (entry == ASSESS) {
            std::vector<uint32_t> kept(n, 77);
            std::vector<double> lrmsd(n, -1.0), irmsd(n, -1.0);
            status = ld_complex_assess(c, n, P, stride, kept.data(), decoy ? lrmsd.data() : nullptr, irmsd.data());
            append(out, kept), append(out, lrmsd), append(out, irmsd);
        } else {
            std::vector<uint32_t> counts(6, 77);
            status = ld_complex_reference_counts(c, counts.data());
            std::vector<uint32_t> pairs(status == LD_OK ? 2 * (size_t)counts[2] : 0, 77);
            if (status == LD_OK) status = ld_complex_native_pairs(c, pairs.data());
            append(out, counts), append(out, pairs);
        }
        break;
    }
    case WRITE_PDB: {
        const std::string path = W.scratch + "/history_model.pdb";
        status = ld_complex_write_pdb(c, P, path.c_str());
        if (status == LD_OK) {
            std::ifstream in(path, std::ios::binary);
            out.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
        }
        break;
    }
    default:
        break;
    }
    return status;
}

// Whether the entry has the refusal at all: no pose (set_reference), no stride (write_pdb), no coordinate bound.
static bool refuses(int entry, int how) {
    if (entry == SET_REFERENCE) return false;
    if (how == STRIDE) return entry != WRITE_PDB;
    if (how == FAR) return entry != COORDINATES && entry != WRITE_PDB;
    return true;
}
// The far pose is found by a kernel.  The stubs of cluster, contacts and assess pose nothing and so find nothing: those three
// calls are made all the same, for what they leave behind, and answer as they may.
static bool stub_finds_far(int entry) { return entry != CLUSTER && entry != CONTACTS && entry != ASSESS; }

struct Fresh {
    Bytes probe[N_ENTRIES];
};

static void probes(ld_complex *c, const Fresh &fresh, const char *after) {
    Bytes out;
    for (int y = 0; y < N_ENTRIES; y++) {
        const bool ok = run(c, y, 0, GOOD, out) == LD_OK && out == fresh.probe[y];
        if (!ok) std::fprintf(stderr, "history_check: probe %s after %s\n", NAMES[y], after);
        CHECK(ok);
    }
}

static void decoys(ld_complex *c) {
    Bytes out;
    for (int x = 0; x < N_ENTRIES; x++) {
        const bool ok = run(c, x, 1, GOOD, out) == LD_OK && !out.empty();
        if (!ok) std::fprintf(stderr, "history_check: decoy %s\n", NAMES[x]);
        CHECK(ok);
    }
    CHECK(run(c, CROSSLINKS, 2, GOOD, out) == LD_OK);
}

static ld_complex *histories(bool flex, Fresh &fresh) {
    Bytes out;
    // what every probe gives on a handle that has run nothing else
    for (int y = 0; y < N_ENTRIES; y++) {
        ld_complex *c = make(flex);
        CHECK(c != nullptr);
        if (!c) return nullptr;
        CHECK(ld_complex_pose_len(c) == (flex ? 11u : 9u));
        CHECK(run(c, y, 0, GOOD, fresh.probe[y]) == LD_OK && !fresh.probe[y].empty());
        CHECK(run(c, y, 0, GOOD, out) == LD_OK && out == fresh.probe[y]);
        ld_complex_destroy(c);
    }
    ld_complex *c = make(flex);
    CHECK(c != nullptr);
    if (!c) return nullptr;
    // 1. the soak; 2. every ordered pair
    decoys(c);
    for (int x = 0; x < N_ENTRIES; x++)
        for (int y = 0; y < N_ENTRIES; y++) {
            CHECK(run(c, x, 1, GOOD, out) == LD_OK);
            const bool ok = run(c, y, 0, GOOD, out) == LD_OK && out == fresh.probe[y];
            if (!ok) std::fprintf(stderr, "history_check: probe %s after decoy %s\n", NAMES[y], NAMES[x]);
            CHECK(ok);
        }
    // 3. refusals as history
    for (int how = FAR; how <= ZERO_QUATERNION; how++)
        for (int x = 0; x < N_ENTRIES; x++) {
            if (!refuses(x, how)) continue;
            const int status = run(c, x, 1, how, out);
            const bool refused = status == LD_ERR_INVALID || (how == FAR && !stub_finds_far(x) && status == LD_OK);
            if (!refused) std::fprintf(stderr, "history_check: decoy %s, refusal %d\n", NAMES[x], how);
            CHECK(refused);
            probes(c, fresh, NAMES[x]);
        }
    CHECK(run(c, ASSESS, 1, GOOD, out) == LD_OK);
    CHECK(ld_complex_set_reference(c, W.ref_b[0].c_str(), W.ref_b[1].c_str(), 0.001, 12.0) == LD_ERR_INVALID);   // no native pair
    uint32_t kept[PROBE_N];
    const std::vector<double> p = poses_of(ASSESS, 0, PROBE_N, ld_complex_pose_len(c), ld_complex_pose_len(c), false);
    CHECK(ld_complex_assess(c, PROBE_N, p.data(), ld_complex_pose_len(c), kept, nullptr, nullptr) == LD_ERR_INVALID);      // and no reference
    CHECK(run(c, SET_REFERENCE, 0, GOOD, out) == LD_OK && out == fresh.probe[SET_REFERENCE]);
    CHECK(run(c, ASSESS, 0, GOOD, out) == LD_OK && out == fresh.probe[ASSESS]);
    // 5. growth, on a handle of its own
    ld_complex *young = make(flex);
    CHECK(young != nullptr);
    if (young) {
        probes(young, fresh, "nothing");
        decoys(young);
        probes(young, fresh, "every decoy");
        ld_complex_destroy(young);
    }
    return c;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: history_check <scratch dir>\n");
        return 2;
    }
    W.scratch = argv[1];
    W.rec = W.scratch + "/history_rec.pdb", W.lig = W.scratch + "/history_lig.pdb";
    put(W.rec, side_text(false, -1, 0.0));
    put(W.lig, side_text(true, -1, 0.0));
    // reference A: the complex itself; B: elsewhere, without a receptor residue and a ligand residue
    W.ref_a[0] = W.rec, W.ref_a[1] = W.lig;
    W.ref_b[0] = W.scratch + "/history_refb_rec.pdb", W.ref_b[1] = W.scratch + "/history_refb_lig.pdb";
    put(W.ref_b[0], side_text(false, 4, 25.0));
    put(W.ref_b[1], side_text(true, 2, 25.0));
    Lcg g(5);
    W.rec_modes.resize(2 * (size_t)N_REC * 3);
    W.lig_modes.resize(2 * (size_t)N_LIG * 3);
    for (double &v : W.rec_modes) v = 0.4 * g.next();
    for (double &v : W.lig_modes) v = 0.4 * g.next();
    // two maps of two shapes
    const uint32_t n0[3] = {9, 6, 5}, n1[3] = {5, 4, 6}, step0[3] = {3000, 3000, 3000}, step1[3] = {4000, 5000, 3500};
    const int32_t origin0[3] = {-2000, -6000, -6000}, origin1[3] = {-5000, -8000, -9000};
    std::vector<float> rho0(9 * 6 * 5), rho1(5 * 4 * 6);
    for (float &v : rho0) v = (float)(0.5 + 0.5 * g.next());
    for (float &v : rho1) v = (float)(1.0 + g.next());
    W.map[0] = ld_density_create(rho0.data(), n0, origin0, step0, 0.3);
    W.map[1] = ld_density_create(rho1.data(), n1, origin1, step1, 0.5);
    CHECK(W.map[0] != nullptr && W.map[1] != nullptr);
    if (W.map[0] && W.map[1]) {
        Fresh fresh[2];
        ld_complex *flex = histories(true, fresh[0]), *rigid = histories(false, fresh[1]);
        // 6. the two handles turn by turn through history 2's first row, the maps one object for both
        if (flex && rigid) {
            Bytes out;
            for (int y = 0; y < N_ENTRIES; y++)
                for (int h = 0; h < 2; h++) {
                    ld_complex *c = h ? rigid : flex;
                    CHECK(run(c, COORDINATES, 1, GOOD, out) == LD_OK);
                    CHECK(run(c, y, 0, GOOD, out) == LD_OK && out == fresh[h].probe[y]);
                }
        }
        if (flex) ld_complex_destroy(flex);
        if (rigid) ld_complex_destroy(rigid);
    }
    ld_density_destroy(W.map[0]);
    ld_density_destroy(W.map[1]);
    std::printf("history_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
