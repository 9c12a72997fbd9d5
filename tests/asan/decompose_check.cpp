// decompose_check.cpp -- driver of the sanitizer build around the energy decomposition (`make asan-decompose`;
// tests/test_asan_decompose.py): ld_scorer_decompose through the C ABI against tests/asan/hip_stub.cpp and
// tests/asan/hip_stub_decompose.cpp (device memory = host memory; the decompose launches do their kernels' work in plain
// C++), so the host's checks, CSR building, workspace carving, passes and copies run under ASan + UBSan and their outputs
// are compared, bit for bit, with a sequential loop written here from the definition in include/lightdock_hip.h: synthetic
// DFIRE and DNA complexes with ANM, restraints and beads; n = 0, 1, 2 and slice + 1; NULL for each optional pointer;
// non-contiguous and empty groups and LD_GROUP_NONE; every refusal by status with the outputs left as they were.
//   usage: decompose_check
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#define CHECK_PROGRAM "decompose_check"
#include "check.hpp"

static uint64_t seed = 88172645463325252ull;
static double uniform() {   // [0, 1)
    seed ^= seed << 13, seed ^= seed >> 7, seed ^= seed << 17;
    return (double)(seed >> 11) / 9007199254740992.0;
}

struct Mol {
    size_t n = 0, num_anm = 0;
    std::vector<double> xyz, q, eps, rad, modes;
    std::vector<uint32_t> types, membrane, offsets, atoms;
    ld_molecule view(bool dfire) const {
        ld_molecule m;
        std::memset(&m, 0, sizeof m);
        m.n_atoms = n;
        m.coordinates = xyz.data();
        if (dfire) {
            m.dfire_types = types.data();
        } else {
            m.ele_charges = q.data();
            m.vdw_charges = eps.data();
            m.vdw_radii = rad.data();
        }
        m.n_membrane = membrane.size();
        m.membrane = membrane.data();
        m.n_restraint_groups = offsets.empty() ? 0 : offsets.size() - 1;
        m.restraint_offsets = offsets.data();
        m.restraint_atoms = atoms.data();
        m.num_anm = num_anm;
        m.nmodes = modes.empty() ? nullptr : modes.data();
        return m;
    }
};

static Mol random_molecule(size_t n, size_t num_anm, double box) {
    Mol m;
    m.n = n;
    m.num_anm = num_anm;
    for (size_t i = 0; i < n; i++) {
        for (int k = 0; k < 3; k++) m.xyz.push_back(box * uniform());
        m.types.push_back((uint32_t)(168.0 * uniform()));
        m.q.push_back(uniform() - 0.5);
        m.eps.push_back(0.01 + 0.2 * uniform());
        m.rad.push_back(1.0 + uniform());
    }
    for (size_t i = 0; i < num_anm * n * 3; i++) m.modes.push_back(uniform() - 0.5);
    return m;
}

// ---- the definition, sequentially -----------------------------------------------------------------------------------
static void qmul(const double a[4], const double b[4], double o[4]) {   // src/qt.rs:174-185
    o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
    o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}
static std::vector<double> posed(const Mol &m, bool ligand, const double *row, const double *ext, bool use_anm) {
    std::vector<double> c = m.xyz;
    for (size_t i = 0; i < m.n; i++) {
        if (ligand) {
            const double *q = row + 3;
            const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
            const double inv[4] = {q[0] / n2, -q[1] / n2, -q[2] / n2, -q[3] / n2}, v[4] = {0.0, c[3 * i], c[3 * i + 1], c[3 * i + 2]};
            double qv[4], r[4];
            qmul(q, v, qv);
            qmul(qv, inv, r);
            for (int k = 0; k < 3; k++) c[3 * i + k] = r[k + 1] + row[k];
        }
        if (use_anm)
            for (size_t k = 0; k < m.num_anm; k++)
                for (int x = 0; x < 3; x++) c[3 * i + x] += m.modes[k * m.n * 3 + i * 3 + x] * ext[k];
    }
    return c;
}
static int dfire_bin(double d2) {   // DIST_TO_BINS[(sqrt(d2) * 2 - 1) as usize] - 1, src/dfire.rs:49-53,336-337
    const double d = std::sqrt(d2) * 2.0 - 1.0;
    const size_t idx = d > 0.0 ? (size_t)d : 0;
    const int v = idx < 3 ? 1 : idx < 15 ? (int)idx - 1 : 14 + (int)(idx - 15) / 2;
    return v - 1;
}

struct Expect {
    std::vector<double> sums[2];        // [side][atom][2]
    std::vector<uint32_t> pairs[2], flag[2];
    ld_energy_terms terms;
};

static Expect expect(bool dfire, bool use_anm, const Mol &R, const Mol &L, const std::vector<double> &table, const double *row) {
    const size_t ar = use_anm ? R.num_anm : 0;
    const std::vector<double> rc = posed(R, false, row, row + 7, use_anm), lc = posed(L, true, row, row + 7 + ar, use_anm);
    Expect e;
    const Mol *mol[2] = {&R, &L};
    for (int side = 0; side < 2; side++) {
        e.sums[side].assign(2 * mol[side]->n, 0.0);
        e.pairs[side].assign(mol[side]->n, 0);
        e.flag[side].assign(mol[side]->n, 0);
        const Mol &own = *mol[side], &oth = *mol[1 - side];
        for (size_t a = 0; a < own.n; a++)
            for (size_t b = 0; b < oth.n; b++) {
                const size_t i = side ? b : a, j = side ? a : b;
                const double dx = rc[3 * i] - lc[3 * j], dy = rc[3 * i + 1] - lc[3 * j + 1], dz = rc[3 * i + 2] - lc[3 * j + 2];
                const double d2 = dx * dx + dy * dy + dz * dz;
                if (dfire) {
                    if (d2 <= 225.0) {
                        e.sums[side][2 * a] += table[(size_t)R.types[i] * 3380 + (size_t)L.types[j] * 20 + (size_t)dfire_bin(d2)];
                        e.pairs[side][a]++;
                        if (std::sqrt(d2) * 2.0 - 1.0 <= 3.9) e.flag[side][a] = 1;
                    }
                } else {
                    if (d2 <= 900.0) {
                        double el = R.q[i] * L.q[j] / d2;
                        if (el > 4.0 / 332.0) el = 4.0 / 332.0;
                        if (el < -4.0 / 332.0) el = -4.0 / 332.0;
                        e.sums[side][2 * a] += el;
                        e.pairs[side][a]++;
                    }
                    if (d2 <= 100.0) {
                        const double rr = R.rad[i] + L.rad[j], rr2 = rr * rr, p6 = rr2 * (rr2 * rr2) / (d2 * d2 * d2);
                        double k = std::sqrt(R.eps[i] * L.eps[j]) * (p6 * p6 - 2.0 * p6);
                        if (k > 1.0) k = 1.0;
                        e.sums[side][2 * a + 1] += k;
                    }
                    if (d2 <= 3.9 * 3.9) e.flag[side][a] = 1;
                }
            }
    }
    ld_energy_terms &t = e.terms;
    std::memset(&t, 0, sizeof t);
    for (size_t a = 0; a < R.n; a++) {
        t.pair[0] += e.sums[0][2 * a];
        t.pair[1] += e.sums[0][2 * a + 1];
        t.pairs += e.pairs[0][a];
        t.rec_interface += e.flag[0][a];
    }
    for (size_t a = 0; a < L.n; a++) t.lig_interface += e.flag[1][a];
    t.score = dfire ? (t.pair[0] * 0.0157 - 4.7) * -1.0 : (t.pair[0] * 332.0 / 4.0 + t.pair[1]) * -1.0;
    double frac[2] = {0.0, 0.0};
    for (int side = 0; side < 2; side++) {
        const Mol &m = *mol[side];
        if (m.offsets.size() < 2) continue;
        size_t hit = 0;
        for (size_t g = 0; g + 1 < m.offsets.size(); g++)
            for (uint32_t k = m.offsets[g]; k < m.offsets[g + 1]; k++)
                if (e.flag[side][m.atoms[k]]) {
                    hit++;
                    break;
                }
        frac[side] = (double)hit / (double)(m.offsets.size() - 1);
    }
    t.rec_restraints = frac[0];
    t.lig_restraints = frac[1];
    double penalty = 0.0;
    if (!R.membrane.empty()) {
        size_t beads = 0;
        for (uint32_t a : R.membrane) beads += e.flag[0][a];
        t.membrane = (double)beads / (double)R.membrane.size();
        if (t.membrane > 0.0) penalty = 999.0 * t.membrane;
    }
    t.energy = t.score + t.rec_restraints * t.score + t.lig_restraints * t.score - penalty;
    return e;
}

static bool same(double a, double b) { return a == b || (a != a && b != b); }
static bool same_terms(const ld_energy_terms &a, const ld_energy_terms &b) {
    return same(a.pair[0], b.pair[0]) && same(a.pair[1], b.pair[1]) && same(a.score, b.score) && same(a.rec_restraints, b.rec_restraints) &&
           same(a.lig_restraints, b.lig_restraints) && same(a.membrane, b.membrane) && same(a.energy, b.energy) && a.pairs == b.pairs &&
           a.rec_interface == b.rec_interface && a.lig_interface == b.lig_interface && a.reserved == 0;
}

// One side's outputs of a call, prefilled so that "untouched" can be told.
struct Out {
    std::vector<double> sums;
    std::vector<uint32_t> pairs, iface;
    Out(size_t n, size_t g) : sums(n * g * 2, -7.5), pairs(n * g, 77u), iface(n * g, 77u) {}
    bool untouched() const {
        for (double v : sums)
            if (v != -7.5) return false;
        for (uint32_t v : pairs)
            if (v != 77u) return false;
        for (uint32_t v : iface)
            if (v != 77u) return false;
        return true;
    }
};

static std::vector<double> random_poses(size_t n, size_t stride, size_t pose_len, double reach) {
    std::vector<double> p(n * stride, std::numeric_limits<double>::quiet_NaN());   // the padding is never read
    for (size_t i = 0; i < n; i++) {
        double *row = &p[i * stride];
        for (int k = 0; k < 3; k++) row[k] = reach * (uniform() - 0.5);
        for (int k = 3; k < 7; k++) row[k] = uniform() - 0.5;   // not a unit quaternion: the inverse divides by |q|^2
        for (size_t k = 7; k < pose_len; k++) row[k] = 2.0 * (uniform() - 0.5);
    }
    return p;
}

static void run_complex(bool dfire, bool use_anm) {
    Mol R = random_molecule(70, 2, 24.0), L = random_molecule(37, 3, 24.0);
    R.membrane = {3, 68, 69};
    R.offsets = {0, 2, 2, 5};   // the middle group is empty
    R.atoms = {0, 40, 69, 1, 2};
    L.offsets = {0, 1};
    L.atoms = {36};
    std::vector<double> table;
    if (dfire)
        for (size_t i = 0; i < (size_t)LD_DFIRE_TABLE_LEN; i++) table.push_back(4.0 * (uniform() - 0.5));
    ld_scorer_desc desc;
    std::memset(&desc, 0, sizeof desc);
    desc.method = dfire ? LD_METHOD_DFIRE : LD_METHOD_DNA;
    desc.use_anm = use_anm;
    desc.receptor = R.view(dfire);
    desc.ligand = L.view(dfire);
    desc.potential = dfire ? table.data() : nullptr;
    ld_scorer *s = ld_scorer_create(&desc);
    CHECK(s != nullptr);
    if (!s) return;
    const size_t pose_len = ld_scorer_pose_len(s), stride = pose_len + 3;
    CHECK(pose_len == (use_anm ? 12u : 7u));
    size_t slice = 0;
    double ms = -1.0;
    CHECK(ld_scorer_decompose_info(s, &slice, &ms) == LD_OK && slice >= 1 && slice <= 4096 && ms == 0.0);
    CHECK(ld_scorer_decompose_info(s, nullptr, nullptr) == LD_OK);

    // groups: a non-contiguous map with an empty group and atoms of no group, on both sides
    const size_t rg = 5, lg = 4;
    std::vector<uint32_t> rmap(R.n), lmap(L.n);
    for (size_t a = 0; a < R.n; a++) rmap[a] = a % 7 == 3 ? LD_GROUP_NONE : (uint32_t)((a * 3) % 4);        // group 4 is empty
    for (size_t a = 0; a < L.n; a++) lmap[a] = a % 5 == 0 ? LD_GROUP_NONE : (uint32_t)(a % 2 ? 3 : 0);      // groups 1, 2 are empty

    const size_t sizes[] = {0, 1, 2, slice + 1};
    for (size_t n : sizes) {
        const std::vector<double> poses = random_poses(n, stride, pose_len, 30.0);
        std::vector<ld_energy_terms> terms(n);
        if (n) std::memset(terms.data(), 0x5a, n * sizeof(ld_energy_terms));
        Out ratoms(n, R.n), latoms(n, L.n), rgrp(n, rg), lgrp(n, lg);
        const ld_group_energies ra = {nullptr, 12345, ratoms.sums.data(), ratoms.pairs.data(), ratoms.iface.data()};   // n_groups ignored without a map
        const ld_group_energies la = {nullptr, 0, latoms.sums.data(), latoms.pairs.data(), latoms.iface.data()};
        CHECK(ld_scorer_decompose(s, n, n ? poses.data() : nullptr, stride, n ? terms.data() : nullptr, &ra, &la) == LD_OK);
        const ld_group_energies rgr = {rmap.data(), rg, rgrp.sums.data(), rgrp.pairs.data(), rgrp.iface.data()};
        const ld_group_energies lgr = {lmap.data(), lg, lgrp.sums.data(), lgrp.pairs.data(), lgrp.iface.data()};
        CHECK(ld_scorer_decompose(s, n, n ? poses.data() : nullptr, stride, nullptr, &rgr, &lgr) == LD_OK);
        int bad = 0;
        for (size_t p = 0; p < n; p++) {
            const Expect e = expect(dfire, use_anm, R, L, table, &poses[p * stride]);
            bad += !same_terms(terms[p], e.terms);
            const Mol *mol[2] = {&R, &L};
            const Out *atoms[2] = {&ratoms, &latoms}, *grp[2] = {&rgrp, &lgrp};
            const std::vector<uint32_t> *map[2] = {&rmap, &lmap};
            const size_t ng[2] = {rg, lg};
            for (int side = 0; side < 2; side++) {
                const size_t na = mol[side]->n;
                std::vector<double> gs(2 * ng[side], 0.0);
                std::vector<uint32_t> gp(ng[side], 0), gi(ng[side], 0);
                for (size_t a = 0; a < na; a++) {
                    bad += !same(atoms[side]->sums[(p * na + a) * 2], e.sums[side][2 * a]) || !same(atoms[side]->sums[(p * na + a) * 2 + 1], e.sums[side][2 * a + 1]);
                    bad += atoms[side]->pairs[p * na + a] != e.pairs[side][a] || atoms[side]->iface[p * na + a] != e.flag[side][a];
                    const uint32_t g = (*map[side])[a];
                    if (g == LD_GROUP_NONE) continue;
                    gs[2 * g] += e.sums[side][2 * a];
                    gs[2 * g + 1] += e.sums[side][2 * a + 1];
                    gp[g] += e.pairs[side][a];
                    gi[g] += e.flag[side][a];
                }
                for (size_t g = 0; g < ng[side]; g++) {
                    bad += !same(grp[side]->sums[(p * ng[side] + g) * 2], gs[2 * g]) || !same(grp[side]->sums[(p * ng[side] + g) * 2 + 1], gs[2 * g + 1]);
                    bad += grp[side]->pairs[p * ng[side] + g] != gp[g] || grp[side]->iface[p * ng[side] + g] != gi[g];
                }
            }
        }
        CHECK(bad == 0);
        if (n) CHECK(ld_scorer_decompose_info(s, nullptr, &ms) == LD_OK && ms >= 0.0);
    }

    // NULL for each optional pointer: what is asked for is the same as before, what is not is never written
    {
        const size_t n = 3;
        const std::vector<double> poses = random_poses(n, stride, pose_len, 20.0);
        std::vector<ld_energy_terms> want(n), got(n);
        Out full(n, rg);
        const ld_group_energies all = {rmap.data(), rg, full.sums.data(), full.pairs.data(), full.iface.data()};
        CHECK(ld_scorer_decompose(s, n, poses.data(), stride, want.data(), &all, nullptr) == LD_OK);
        CHECK(ld_scorer_decompose(s, n, poses.data(), stride, got.data(), nullptr, nullptr) == LD_OK);
        for (size_t p = 0; p < n; p++) CHECK(same_terms(want[p], got[p]));
        CHECK(ld_scorer_decompose(s, n, poses.data(), stride, nullptr, nullptr, nullptr) == LD_OK);
        for (int drop = 0; drop < 3; drop++) {
            Out part(n, rg);
            const ld_group_energies g = {rmap.data(), rg, drop == 0 ? nullptr : part.sums.data(), drop == 1 ? nullptr : part.pairs.data(),
                                         drop == 2 ? nullptr : part.iface.data()};
            CHECK(ld_scorer_decompose(s, n, poses.data(), stride, nullptr, &g, nullptr) == LD_OK);
            CHECK(drop == 0 ? part.sums == Out(n, rg).sums : std::memcmp(part.sums.data(), full.sums.data(), part.sums.size() * sizeof(double)) == 0);
            CHECK(drop == 1 ? part.pairs == Out(n, rg).pairs : part.pairs == full.pairs);
            CHECK(drop == 2 ? part.iface == Out(n, rg).iface : part.iface == full.iface);
        }
        const ld_group_energies nothing = {rmap.data(), rg, nullptr, nullptr, nullptr};
        CHECK(ld_scorer_decompose(s, n, poses.data(), stride, nullptr, &nothing, &nothing) == LD_OK);
    }

    // refusals: status, a message, every output as it was
    {
        const size_t n = 4;
        const std::vector<double> poses = random_poses(n, stride, pose_len, 20.0);
        std::vector<ld_energy_terms> terms(n);
        std::memset(terms.data(), 0x5a, n * sizeof(ld_energy_terms));
        const std::vector<ld_energy_terms> before = terms;
        Out ro(n, rg), lo(n, lg);
        auto refused = [&](size_t count, size_t st, const uint32_t *rm, size_t rgroups, const uint32_t *lm, size_t lgroups) {
            const ld_group_energies r = {rm, rgroups, ro.sums.data(), ro.pairs.data(), ro.iface.data()};
            const ld_group_energies l = {lm, lgroups, lo.sums.data(), lo.pairs.data(), lo.iface.data()};
            const int rc = ld_scorer_decompose(s, count, poses.data(), st, terms.data(), &r, &l);
            CHECK(rc == LD_ERR_INVALID && std::strlen(ld_last_error()) > 0 && ro.untouched() && lo.untouched() &&
                  std::memcmp(terms.data(), before.data(), n * sizeof(ld_energy_terms)) == 0);
        };
        refused(n, pose_len - 1, rmap.data(), rg, lmap.data(), lg);          // stride below the pose length
        refused(n, stride, rmap.data(), rg - 2, lmap.data(), lg);            // a receptor group id >= n_groups
        refused(n, stride, rmap.data(), rg, lmap.data(), lg - 1);            // a ligand group id >= n_groups
        refused(n, stride, rmap.data(), 0, lmap.data(), lg);                 // n_groups = 0 with a map
        refused(n, stride, rmap.data(), rg, lmap.data(), 0);
        refused(std::numeric_limits<size_t>::max() / 8, stride, rmap.data(), rg, lmap.data(), lg);   // n x n_groups overflows (n x stride too)
        refused(std::numeric_limits<size_t>::max() / 16 / R.n + 1, stride, nullptr, 0, lmap.data(), lg);   // n x n_atoms under a NULL map; n x stride fits
        {   // a map is checked even where none of its rows is asked for
            const ld_group_energies bad_ids = {rmap.data(), rg - 2, nullptr, nullptr, nullptr}, no_groups = {rmap.data(), 0, nullptr, nullptr, nullptr};
            CHECK(ld_scorer_decompose(s, n, poses.data(), stride, terms.data(), &bad_ids, nullptr) == LD_ERR_INVALID);
            CHECK(ld_scorer_decompose(s, n, poses.data(), stride, terms.data(), nullptr, &no_groups) == LD_ERR_INVALID);
            CHECK(std::memcmp(terms.data(), before.data(), n * sizeof(ld_energy_terms)) == 0);
        }
        CHECK(ld_scorer_decompose(nullptr, n, poses.data(), stride, terms.data(), nullptr, nullptr) == LD_ERR_INVALID);
        CHECK(ld_scorer_decompose(s, n, nullptr, stride, terms.data(), nullptr, nullptr) == LD_ERR_INVALID);
        CHECK(std::memcmp(terms.data(), before.data(), n * sizeof(ld_energy_terms)) == 0);
        CHECK(ld_scorer_decompose_info(nullptr, &slice, &ms) == LD_ERR_INVALID);
        // and the scorer still serves
        CHECK(ld_scorer_decompose(s, n, poses.data(), stride, terms.data(), nullptr, nullptr) == LD_OK);
        CHECK(same_terms(terms[n - 1], expect(dfire, use_anm, R, L, table, &poses[(n - 1) * stride]).terms));
    }
    ld_scorer_destroy(s);
}

int main() {
    run_complex(true, false);
    run_complex(true, true);
    run_complex(false, true);
    run_complex(false, false);
    std::printf("decompose_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
