#include "decompose.hpp"

#include <algorithm>
#include <climits>
#include <cstring>
#include <limits>

#include "scorer.hpp"

namespace ld {

// ---------------------------------------------------------------------------------------
// DescCopy
// ---------------------------------------------------------------------------------------
void DescCopy::copy(const ld_molecule &from, Molecule &store, ld_molecule &to) {
    const size_t n = from.n_atoms;
    auto take = [](auto &vec, const auto *src, size_t count) {
        if (src && count) vec.assign(src, src + count);
        return vec.empty() ? nullptr : vec.data();
    };
    to = from;
    to.coordinates = take(store.coordinates, from.coordinates, 3 * n);
    to.dfire_types = take(store.dfire_types, from.dfire_types, n);
    to.ele_charges = take(store.ele_charges, from.ele_charges, n);
    to.vdw_charges = take(store.vdw_charges, from.vdw_charges, n);
    to.vdw_radii = take(store.vdw_radii, from.vdw_radii, n);
    to.membrane = take(store.membrane, from.membrane, from.n_membrane);
    to.restraint_offsets = take(store.restraint_offsets, from.restraint_offsets, from.n_restraint_groups ? from.n_restraint_groups + 1 : 0);
    to.restraint_atoms = take(store.restraint_atoms, from.restraint_atoms, store.restraint_offsets.empty() ? 0 : store.restraint_offsets.back());
    to.nmodes = take(store.nmodes, from.nmodes, from.num_anm * n * 3);
}

DescCopy::DescCopy(const ld_scorer_desc &d) {
    desc_ = d;
    copy(d.receptor, rec_, desc_.receptor);
    copy(d.ligand, lig_, desc_.ligand);
    if (d.potential && d.method == LD_METHOD_DFIRE) potential_.assign(d.potential, d.potential + LD_DFIRE_TABLE_LEN);
    desc_.potential = potential_.empty() ? nullptr : potential_.data();
}

// ---------------------------------------------------------------------------------------
// Decomposer
// ---------------------------------------------------------------------------------------
namespace {

int padded(size_t n) { return (int)((n + 63) / 64 * 64); }
bool flexes(const ld_scorer_desc &desc, const ld_molecule &m) { return desc.use_anm != 0 && m.num_anm > 0; }

}  // namespace

size_t Decomposer::slice_of(const ld_scorer_desc &desc) {
    return decompose_slice(padded(desc.receptor.n_atoms), padded(desc.ligand.n_atoms), flexes(desc, desc.receptor));
}

DecomposeMolecule Decomposer::upload(const ld_molecule &m, int method, bool is_receptor, bool use_anm) {
    const size_t n = m.n_atoms, n_pad = (size_t)padded(n);
    DecomposeMolecule dev;
    dev.n = (int)n;
    dev.n_pad = (int)n_pad;
    std::vector<double> x(n_pad, 0.0), y(n_pad, 0.0), z(n_pad, 0.0);
    for (size_t i = 0; i < n; i++) {
        x[i] = m.coordinates[3 * i];
        y[i] = m.coordinates[3 * i + 1];
        z[i] = m.coordinates[3 * i + 2];
    }
    dev.x = arena_.upload(x);
    dev.y = arena_.upload(y);
    dev.z = arena_.upload(z);
    if (method == LD_METHOD_DFIRE) {
        std::vector<uint32_t> t(n_pad, 0);   // potential[atoma*169*20 + atomb*20 + bin], src/dfire.rs:338
        for (size_t i = 0; i < n; i++) t[i] = m.dfire_types[i] * (is_receptor ? kDfireRowStride : 20u);
        dev.tindex = arena_.upload(t);
    } else {
        dev.charge = arena_.upload(std::vector<double>(m.ele_charges, m.ele_charges + n), n_pad);
        dev.eps = arena_.upload(std::vector<double>(m.vdw_charges, m.vdw_charges + n), n_pad);
        dev.radius = arena_.upload(std::vector<double>(m.vdw_radii, m.vdw_radii + n), n_pad);
    }
    if (use_anm && m.num_anm > 0) {   // (mode, atom, xyz) -> [mode][xyz][n_pad]
        std::vector<double> modes(m.num_anm * 3 * n_pad, 0.0);
        for (size_t k = 0; k < m.num_anm; k++)
            for (size_t i = 0; i < n; i++)
                for (int c = 0; c < 3; c++) modes[(k * 3 + c) * n_pad + i] = m.nmodes[k * n * 3 + i * 3 + c];
        dev.modes = arena_.upload(modes);
        dev.num_anm = (int)m.num_anm;
    }
    return dev;
}

Decomposer::Decomposer(const ld_scorer_desc &desc) {
    const int method = desc.method == LD_METHOD_PYDOCK ? LD_METHOD_DNA : desc.method;   // src/pydock.rs:425-545 == src/dna.rs:411-529
    const bool use_anm = desc.use_anm != 0;
    DecomposeLaunch &D = model_;
    D.method = method;
    D.rec = upload(desc.receptor, method, true, use_anm);
    D.lig = upload(desc.ligand, method, false, use_anm);
    D.iface_d2 = 3.9 * 3.9;   // INTERFACE_CUTOFF2, src/constants.rs:15
    if (method == LD_METHOD_DFIRE) {
        if (!desc.potential) throw Error(LD_ERR_IO, "Unable to open DFIRE parameters");
        const DfireBinning binning = build_dfire_binning();
        D.table = arena_.upload(std::vector<double>(desc.potential, desc.potential + LD_DFIRE_TABLE_LEN));
        D.lut = arena_.upload(binning.lut);
        D.bin_step = arena_.upload(binning.step);
        D.iface_d2 = dfire_interface_d2();
    }
    auto csr = [&](const ld_molecule &m, const uint32_t **offsets, const uint32_t **atoms) {
        std::vector<uint32_t> o(1, 0), a;
        if (m.n_restraint_groups) {
            o.assign(m.restraint_offsets, m.restraint_offsets + m.n_restraint_groups + 1);
            a.assign(m.restraint_atoms, m.restraint_atoms + o.back());
        }
        *offsets = arena_.upload(o);
        *atoms = arena_.upload(a);
        return (int)m.n_restraint_groups;
    };
    tail_.n_rec_groups = csr(desc.receptor, &tail_.rec_offsets, &tail_.rec_atoms);
    tail_.n_lig_groups = csr(desc.ligand, &tail_.lig_offsets, &tail_.lig_atoms);
    // src/scoring.rs:38-47 is only ever applied to the receptor (src/dfire.rs:357)
    tail_.n_membrane = (int)desc.receptor.n_membrane;
    tail_.membrane = arena_.upload(std::vector<uint32_t>(desc.receptor.membrane, desc.receptor.membrane + desc.receptor.n_membrane));
    slice_ = slice_of(desc);
    hip_check(hipEventCreate(&start_), "hipEventCreate");
    hip_check(hipEventCreate(&stop_), "hipEventCreate");
}

Decomposer::~Decomposer() {
    if (start_) (void)hipEventDestroy(start_);
    if (stop_) (void)hipEventDestroy(stop_);
}

void Decomposer::check_groups(const ld_group_energies *g, int side, size_t n, SideGroups &out) const {
    out.wanted = false;
    if (!g) return;
    const char *who = side ? "ligand" : "receptor";
    const size_t n_atoms = (size_t)(side ? model_.lig.n : model_.rec.n);
    const size_t n_groups = g->group_of_atom ? g->n_groups : n_atoms;
    if (n_groups == 0) throw Error(LD_ERR_INVALID, std::string("ld_scorer_decompose: ") + who + " group map with n_groups = 0");
    if (n_groups > (size_t)INT_MAX || n > std::numeric_limits<size_t>::max() / 16 / n_groups)
        throw Error(LD_ERR_INVALID, std::string("ld_scorer_decompose: ") + who + " n x n_groups overflows");
    out.offsets.assign(n_groups + 1, 0);
    out.atoms.clear();
    if (g->group_of_atom) {
        for (size_t a = 0; a < n_atoms; a++) {
            const uint32_t id = g->group_of_atom[a];
            if (id == LD_GROUP_NONE) continue;
            if (id >= n_groups) throw Error(LD_ERR_INVALID, std::string("ld_scorer_decompose: ") + who + " group id out of range");
            out.offsets[(size_t)id + 1]++;
        }
        for (size_t k = 0; k < n_groups; k++) out.offsets[k + 1] += out.offsets[k];
        out.atoms.resize(out.offsets[n_groups]);
        std::vector<uint32_t> next(out.offsets.begin(), out.offsets.end() - 1);
        for (size_t a = 0; a < n_atoms; a++)   // ascending atom index within every group
            if (g->group_of_atom[a] != LD_GROUP_NONE) out.atoms[next[g->group_of_atom[a]]++] = (uint32_t)a;
    } else {
        out.atoms.resize(n_atoms);
        for (size_t a = 0; a < n_atoms; a++) out.offsets[a + 1] = (uint32_t)(a + 1), out.atoms[a] = (uint32_t)a;
    }
    out.n_groups = n_groups;
    out.wanted = g->sums || g->pairs || g->interface_atoms;   // a map is checked even where no row of it is asked for
}

void Decomposer::run(size_t n, const double *poses, size_t stride, ld_energy_terms *terms_out, const ld_group_energies *receptor,
                     const ld_group_energies *ligand, hipStream_t stream) {
    if (n == 0) return;
    if (!poses) throw Error(LD_ERR_INVALID, "ld_scorer_decompose: poses missing");
    if (stride < pose_len()) throw Error(LD_ERR_INVALID, "ld_scorer_decompose: stride below the pose length");
    const ld_group_energies *asked[2] = {receptor, ligand};
    for (int side = 0; side < 2; side++) check_groups(asked[side], side, n, groups_[side]);
    if (n > std::numeric_limits<size_t>::max() / sizeof(double) / stride) throw Error(LD_ERR_INVALID, "ld_scorer_decompose: n x stride overflows");

    // the workspace of a pass (kernels/decompose.hpp, DecomposeLaunch), carved for `cap` poses: doubles first
    const size_t cap = std::min(n, slice_);
    const size_t nr = (size_t)model_.rec.n_pad, nl = (size_t)model_.lig.n_pad;
    const bool rec_flexes = model_.rec.num_anm > 0;
    ws_.reserve(cap * decompose_pose_bytes(model_.rec.n_pad, model_.lig.n_pad, rec_flexes));
    DecomposeLaunch D = model_;
    {
        double *d = static_cast<double *>(ws_.ptr);
        D.lig_xyz = d, d += cap * 3 * nl;
        if (rec_flexes) D.rec_xyz = d, d += cap * 3 * nr;
        D.rec_sum = d, d += cap * 2 * nr;
        D.lig_sum = d, d += cap * 2 * nl;
        uint32_t *u = reinterpret_cast<uint32_t *>(d);
        D.rec_pairs = u, u += cap * nr;
        D.lig_pairs = u, u += cap * nl;
        D.rec_flag = u, u += cap * nr;
        D.lig_flag = u, u += cap * nl;
    }
    ws_poses_.reserve(((cap - 1) * stride + pose_len()) * sizeof(double));
    if (terms_out) ws_terms_.reserve(cap * sizeof(ld_energy_terms));
    DecomposeGroups G[2];
    for (int side = 0; side < 2; side++) {
        SideGroups &s = groups_[side];
        if (!s.wanted) continue;
        const ld_group_energies &g = *asked[side];
        s.d_offsets.reserve(s.offsets.size() * sizeof(uint32_t));
        s.d_atoms.reserve(std::max<size_t>(1, s.atoms.size()) * sizeof(uint32_t));
        hip_check(hipMemcpyAsync(s.d_offsets.ptr, s.offsets.data(), s.offsets.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream), "hipMemcpy H2D");
        if (!s.atoms.empty())
            hip_check(hipMemcpyAsync(s.d_atoms.ptr, s.atoms.data(), s.atoms.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream), "hipMemcpy H2D");
        G[side].n_groups = (int)s.n_groups;
        G[side].offsets = static_cast<const uint32_t *>(s.d_offsets.ptr);
        G[side].atoms = static_cast<const uint32_t *>(s.d_atoms.ptr);
        if (g.sums) s.d_sums.reserve(cap * s.n_groups * 2 * sizeof(double)), G[side].sums = static_cast<double *>(s.d_sums.ptr);
        if (g.pairs) s.d_pairs.reserve(cap * s.n_groups * sizeof(uint32_t)), G[side].pairs = static_cast<uint32_t *>(s.d_pairs.ptr);
        if (g.interface_atoms) s.d_iface.reserve(cap * s.n_groups * sizeof(uint32_t)), G[side].iface = static_cast<uint32_t *>(s.d_iface.ptr);
    }

    last_ms_ = 0.0;
    for (size_t first = 0; first < n; first += slice_) {
        const size_t m = std::min(slice_, n - first);
        hip_check(hipMemcpyAsync(ws_poses_.ptr, poses + first * stride, ((m - 1) * stride + pose_len()) * sizeof(double), hipMemcpyHostToDevice, stream),
                  "hipMemcpy H2D");
        D.poses = static_cast<const double *>(ws_poses_.ptr);
        D.stride = stride;
        D.n_poses = (int)m;
        hip_check(hipEventRecord(start_, stream), "hipEventRecord");
        hip_check(launch_decompose_pose(D, stream), "launch decompose_pose");
        hip_check(launch_decompose_side(D, 0, stream), "launch decompose_side (receptor)");
        hip_check(launch_decompose_side(D, 1, stream), "launch decompose_side (ligand)");
        for (int side = 0; side < 2; side++)
            if (groups_[side].wanted) hip_check(launch_decompose_groups(D, side, G[side], stream), "launch decompose_groups");
        if (terms_out) hip_check(launch_decompose_terms(D, tail_, static_cast<ld_energy_terms *>(ws_terms_.ptr), stream), "launch decompose_terms");
        hip_check(hipEventRecord(stop_, stream), "hipEventRecord");
        if (terms_out)
            hip_check(hipMemcpyAsync(terms_out + first, ws_terms_.ptr, m * sizeof(ld_energy_terms), hipMemcpyDeviceToHost, stream), "hipMemcpy D2H");
        for (int side = 0; side < 2; side++) {
            if (!groups_[side].wanted) continue;
            const ld_group_energies &g = *asked[side];
            const size_t ng = groups_[side].n_groups;
            if (g.sums) hip_check(hipMemcpyAsync(g.sums + first * ng * 2, G[side].sums, m * ng * 2 * sizeof(double), hipMemcpyDeviceToHost, stream), "hipMemcpy D2H");
            if (g.pairs) hip_check(hipMemcpyAsync(g.pairs + first * ng, G[side].pairs, m * ng * sizeof(uint32_t), hipMemcpyDeviceToHost, stream), "hipMemcpy D2H");
            if (g.interface_atoms)
                hip_check(hipMemcpyAsync(g.interface_atoms + first * ng, G[side].iface, m * ng * sizeof(uint32_t), hipMemcpyDeviceToHost, stream), "hipMemcpy D2H");
        }
        hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
        float ms = 0.f;
        hip_check(hipEventElapsedTime(&ms, start_, stop_), "hipEventElapsedTime");
        last_ms_ += (double)ms;
    }
}

}  // namespace ld
