// hip_stub_decompose.cpp -- TEST INFRASTRUCTURE for the sanitizer build of the host side (`make asan`, `make asan-assess`,
// `make asan-ranked`, `make asan-decompose`): the launches of kernels/decompose.hpp, beside tests/asan/hip_stub.cpp which
// stands in for the HIP runtime and every other kernel.  Device memory is host memory there, so ASan checks every extent
// below against what decompose.cpp allocated and carved.  Like the ranked stubs these DO what their kernels do, in plain
// C++ over kernels/decompose_pair.hpp, so that ld_scorer_decompose's outputs can be checked (tests/asan/decompose_check.cpp);
// each also touches both ends of every buffer its kernel reads or writes, the extents as decompose.hip indexes them.
#include <cstring>

#include "kernels/decompose.hpp"
#include "kernels/decompose_pair.hpp"
#include "kernels/pose_energy.hpp"
#include "stub_access.hpp"

namespace ld {

static void peek_molecule(const DecomposeMolecule &m, bool dfire) {
    const size_t n_pad = (size_t)m.n_pad;
    peek(m.x, n_pad);
    peek(m.y, n_pad);
    peek(m.z, n_pad);
    if (dfire) {
        peek(m.tindex, n_pad);
    } else {
        peek(m.charge, n_pad);
        peek(m.eps, n_pad);
        peek(m.radius, n_pad);
    }
    peek(m.modes, (size_t)m.num_anm * 3 * n_pad);
}

static bool sane(const DecomposeLaunch &d) {
    return d.n_poses >= 1 && d.rec.n >= 1 && d.lig.n >= 1 && d.rec.n_pad >= d.rec.n && d.lig.n_pad >= d.lig.n && d.rec.n_pad % 64 == 0 &&
           d.lig.n_pad % 64 == 0 && d.poses && d.lig_xyz && d.rec_sum && d.lig_sum && d.rec_pairs && d.lig_pairs && d.rec_flag && d.lig_flag &&
           (d.rec.num_anm > 0) == (d.rec_xyz != nullptr);
}

static void peek_inputs(const DecomposeLaunch &d) {
    const bool dfire = d.method == 0;
    peek_molecule(d.rec, dfire);
    peek_molecule(d.lig, dfire);
    if (dfire) {
        peek(d.table, (size_t)LD_DFIRE_TABLE_LEN);
        peek(d.lut, (size_t)kDfireLutCells);
        peek(d.bin_step, (size_t)kDfireSteps);
    }
    peek(d.poses, ((size_t)d.n_poses - 1) * d.stride + 7 + d.rec.num_anm + d.lig.num_anm);   // row p: poses + p * stride
}

hipError_t launch_decompose_pose(const DecomposeLaunch &d, hipStream_t) {
    if (d.n_poses <= 0) return hipSuccess;
    if (!sane(d)) return hipErrorInvalidValue;
    peek_inputs(d);
    const size_t P = (size_t)d.n_poses;
    peek(d.lig_xyz, P * 3 * d.lig.n_pad);
    if (d.rec_xyz) peek(d.rec_xyz, P * 3 * d.rec.n_pad);
    for (size_t p = 0; p < P; p++) {
        const double *row = d.poses + p * d.stride;
        for (int side = 0; side < 2; side++) {
            const DecomposeMolecule &m = side ? d.lig : d.rec;
            double *out = side ? d.lig_xyz : d.rec_xyz;
            if (!out) continue;
            out += p * 3 * (size_t)m.n_pad;
            for (int a = 0; a < m.n; a++) {
                double v[3];
                decompose::pose_atom(side == 1, row, m.x[a], m.y[a], m.z[a], m.num_anm, m.modes, (size_t)m.n_pad, (size_t)a,
                                     row + 7 + (side ? d.rec.num_anm : 0), v);
                for (int k = 0; k < 3; k++) out[(size_t)k * m.n_pad + a] = v[k];
            }
        }
    }
    return hipSuccess;
}

hipError_t launch_decompose_side(const DecomposeLaunch &d, int side, hipStream_t) {
    if (d.n_poses <= 0) return hipSuccess;
    if (!sane(d) || side < 0 || side > 1) return hipErrorInvalidValue;
    peek_inputs(d);
    const size_t P = (size_t)d.n_poses, nr = (size_t)d.rec.n_pad, nl = (size_t)d.lig.n_pad;
    const DecomposeMolecule &own = side ? d.lig : d.rec, &oth = side ? d.rec : d.lig;
    const size_t no = (size_t)own.n_pad;
    double *sum = side ? d.lig_sum : d.rec_sum;
    uint32_t *pairs = side ? d.lig_pairs : d.rec_pairs, *flag = side ? d.lig_flag : d.rec_flag;
    peek(d.lig_xyz, P * 3 * nl);
    if (d.rec_xyz) peek(d.rec_xyz, P * 3 * nr);
    peek(sum, P * 2 * no);
    peek(pairs, P * no);
    peek(flag, P * no);
    for (size_t p = 0; p < P; p++) {
        const double *rx = d.rec_xyz ? d.rec_xyz + p * 3 * nr : d.rec.x, *ry = d.rec_xyz ? rx + nr : d.rec.y, *rz = d.rec_xyz ? ry + nr : d.rec.z;
        const double *lx = d.lig_xyz + p * 3 * nl, *ly = lx + nl, *lz = ly + nl;
        for (int a = 0; a < own.n; a++) {
            double acc0 = 0.0, acc1 = 0.0;
            uint32_t cnt = 0, fl = 0;
            for (int b = 0; b < oth.n; b++) {
                const int i = side ? b : a, j = side ? a : b;   // receptor atom, ligand atom
                const double d2 = decompose::dist2(rx[i], ry[i], rz[i], lx[j], ly[j], lz[j]);
                if (d.method == 0) {
                    if (d2 <= 225.0) {
                        acc0 += d.table[d.rec.tindex[i] + d.lig.tindex[j] + decompose::dfire_bin(d2, d.lut, d.bin_step)];
                        cnt++;
                        if (d2 <= d.iface_d2) fl = 1;
                    }
                } else {
                    if (d2 <= decompose::kElecCutoff2) {
                        acc0 += decompose::dna_elec(d.rec.charge[i], d.lig.charge[j], d2);
                        cnt++;
                    }
                    if (d2 <= decompose::kVdwCutoff2) acc1 += decompose::dna_vdw(d.rec.eps[i], d.lig.eps[j], d.rec.radius[i], d.lig.radius[j], d2);
                    if (d2 <= d.iface_d2) fl = 1;
                }
            }
            sum[p * 2 * no + a] = acc0;
            sum[p * 2 * no + no + a] = acc1;
            pairs[p * no + a] = cnt;
            flag[p * no + a] = fl;
        }
    }
    return hipSuccess;
}

hipError_t launch_decompose_groups(const DecomposeLaunch &d, int side, const DecomposeGroups &g, hipStream_t) {
    if (d.n_poses <= 0 || g.n_groups <= 0) return hipSuccess;
    if (!sane(d) || side < 0 || side > 1 || !g.offsets || !g.atoms) return hipErrorInvalidValue;
    const size_t P = (size_t)d.n_poses, G = (size_t)g.n_groups, n_pad = (size_t)(side ? d.lig.n_pad : d.rec.n_pad);
    const int n = side ? d.lig.n : d.rec.n;
    peek(g.offsets, G + 1);
    peek(g.atoms, (size_t)g.offsets[G]);
    if (g.sums) peek(g.sums, P * G * 2);
    if (g.pairs) peek(g.pairs, P * G);
    if (g.iface) peek(g.iface, P * G);
    const double *sum = side ? d.lig_sum : d.rec_sum;
    const uint32_t *pairs = side ? d.lig_pairs : d.rec_pairs, *flag = side ? d.lig_flag : d.rec_flag;
    for (size_t p = 0; p < P; p++)
        for (size_t k = 0; k < G; k++) {
            double s0 = 0.0, s1 = 0.0;
            uint32_t cnt = 0, fl = 0;
            for (uint32_t q = g.offsets[k]; q < g.offsets[k + 1]; q++) {
                const uint32_t a = g.atoms[q];
                if (a >= (uint32_t)n) return hipErrorInvalidValue;
                s0 += sum[p * 2 * n_pad + a];
                s1 += sum[p * 2 * n_pad + n_pad + a];
                cnt += pairs[p * n_pad + a];
                fl += flag[p * n_pad + a];
            }
            if (g.sums) g.sums[2 * (p * G + k)] = s0, g.sums[2 * (p * G + k) + 1] = s1;
            if (g.pairs) g.pairs[p * G + k] = cnt;
            if (g.iface) g.iface[p * G + k] = fl;
        }
    return hipSuccess;
}

static double fraction(const uint32_t *flag, int n_groups, const uint32_t *offsets, const uint32_t *atoms) {
    if (n_groups == 0) return 0.0;
    int hit = 0;
    for (int g = 0; g < n_groups; g++)
        for (uint32_t k = offsets[g]; k < offsets[g + 1]; k++)
            if (flag[atoms[k]]) {
                hit++;
                break;
            }
    return (double)hit / (double)n_groups;
}

hipError_t launch_decompose_terms(const DecomposeLaunch &d, const DecomposeTail &t, ld_energy_terms *terms, hipStream_t) {
    if (d.n_poses <= 0) return hipSuccess;
    if (!sane(d) || !terms) return hipErrorInvalidValue;
    const size_t P = (size_t)d.n_poses, nr = (size_t)d.rec.n_pad, nl = (size_t)d.lig.n_pad;
    peek(t.rec_offsets, (size_t)t.n_rec_groups + 1);
    peek(t.rec_atoms, (size_t)t.rec_offsets[t.n_rec_groups]);
    peek(t.lig_offsets, (size_t)t.n_lig_groups + 1);
    peek(t.lig_atoms, (size_t)t.lig_offsets[t.n_lig_groups]);
    peek(t.membrane, (size_t)t.n_membrane);
    peek(terms, P);
    for (size_t p = 0; p < P; p++) {
        const double *sum = d.rec_sum + p * 2 * nr;
        const uint32_t *rflag = d.rec_flag + p * nr, *lflag = d.lig_flag + p * nl;
        ld_energy_terms out;
        std::memset(&out, 0, sizeof out);
        for (int a = 0; a < d.rec.n; a++) {
            out.pair[0] += sum[a];
            out.pair[1] += sum[nr + a];
            out.pairs += d.rec_pairs[p * nr + a];
            out.rec_interface += rflag[a];
        }
        for (int a = 0; a < d.lig.n; a++) out.lig_interface += lflag[a];
        if (d.method == 0) {
            out.score = (out.pair[0] * 0.0157 - 4.7) * -1.0;
        } else {
            const double total_elec = out.pair[0] * 332.0 / 4.0;
            out.score = (total_elec + out.pair[1]) * -1.0;
        }
        out.rec_restraints = fraction(rflag, t.n_rec_groups, t.rec_offsets, t.rec_atoms);
        out.lig_restraints = fraction(lflag, t.n_lig_groups, t.lig_offsets, t.lig_atoms);
        double penalty = 0.0;
        if (t.n_membrane > 0) {
            uint32_t beads = 0;
            for (int k = 0; k < t.n_membrane; k++) beads += rflag[t.membrane[k]];
            out.membrane = (double)beads / (double)t.n_membrane;
            if (out.membrane > 0.0) penalty = 999.0 * out.membrane;
        }
        out.energy = out.score + out.rec_restraints * out.score + out.lig_restraints * out.score - penalty;
        terms[p] = out;
    }
    return hipSuccess;
}

}  // namespace ld
