// complex.cpp -- the host side of the analysis half of a run: argument checks, the workspace of every call (each block's
// layout written once, for a Carver; chunks and slots by chunk_of), the launch sequences of kernels/cluster.hpp between
// begin_timed and finish_timed, and ld_complex_write_pdb's text.
#include "complex.hpp"

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>

namespace ld {

namespace {

void check_modes(const char *side, const double *modes, size_t len, size_t num_anm, size_t n_atoms) {
    if (len != num_anm * n_atoms * 3 || (len && !modes))
        throw Error(LD_ERR_INVALID, std::string(side) + ": " + std::to_string(len) +
                                        " mode values, expected num_anm x atoms x 3 = " + std::to_string(num_anm * n_atoms * 3));
}

}  // namespace

long long cutoff_thousandths(double cutoff, const char *message) {
    const double scaled = cutoff * 1000.0;
    if (!(scaled > 0.0 && scaled < 30001.0)) throw Error(LD_ERR_INVALID, message);
    const long long C = std::llrint(scaled);
    if (C < 1 || C > 30000) throw Error(LD_ERR_INVALID, message);
    return C;
}

void check_scoring(size_t n, const double *scoring) {
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(scoring[i])) throw Error(LD_ERR_INVALID, "scoring " + std::to_string(i) + " is not finite");
}

std::string record_element(const char *line, size_t len) {
    std::string element;
    if (len >= 78)
        for (size_t k = 76; k < 78; k++)
            if (line[k] != ' ') element.push_back((char)std::toupper((unsigned char)line[k]));
    if (element.empty())
        for (size_t k = 12; k < 16 && element.empty(); k++)
            if (std::isalpha((unsigned char)line[k])) element.push_back((char)std::toupper((unsigned char)line[k]));
    return element;
}

std::string record_residue_name(const char *line) {
    size_t b = 17, e = 20;
    while (b < e && line[b] == ' ') b++;
    while (e > b && line[e - 1] == ' ') e--;
    return std::string(line + b, e - b);
}

uint32_t sasa_radius(const char *line, size_t len) {
    static const struct {
        const char *element;
        uint32_t radius;
    } table[] = {{"C", 1700}, {"N", 1550}, {"O", 1520}, {"F", 1470}, {"P", 1800}, {"S", 1800}, {"CL", 1750}, {"SE", 1900}, {"BR", 1850}, {"I", 1980}};
    const std::string element = record_element(line, len);
    if (element == "H" || element == "D" || record_residue_name(line) == "MMB") return 0;
    for (const auto &row : table)
        if (element == row.element) return row.radius;
    return 1800;
}

Complex::Complex(const char *receptor_pdb, const char *ligand_pdb, const double *rec_nmodes, size_t rec_nmodes_len,
                 size_t rec_num_anm, const double *lig_nmodes, size_t lig_nmodes_len, size_t lig_num_anm)
    : rec_(read_pdb_file_order(receptor_pdb)), lig_(read_pdb_file_order(ligand_pdb)) {
    check_modes("receptor", rec_nmodes, rec_nmodes_len, rec_num_anm, rec_.lines.size());
    check_modes("ligand", lig_nmodes, lig_nmodes_len, lig_num_anm, lig_.lines.size());
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        throw Error(LD_ERR_DEVICE, "no HIP device available: the analysis path has no CPU fallback");
    int device = 0;
    hip_check(hipGetDevice(&device), "hipGetDevice");
    hipDeviceProp_t prop;
    hip_check(hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        throw Error(LD_ERR_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");

    try {
        hip_check(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking), "hipStreamCreate");
        hip_check(hipEventCreate(&ev0_), "hipEventCreate");
        hip_check(hipEventCreate(&ev1_), "hipEventCreate");
        ComplexDevice &d = dev_;
        d.n_rec = (int)rec_.lines.size();
        d.n_lig = (int)lig_.lines.size();
        d.anm_rec = (int)rec_num_anm;
        d.anm_lig = (int)lig_num_anm;
        d.rec_xyz = arena_.upload(rec_.xyz);
        d.lig_xyz = arena_.upload(lig_.xyz);
        d.rec_modes = arena_.upload(std::vector<double>(rec_nmodes, rec_nmodes + rec_nmodes_len));
        d.lig_modes = arena_.upload(std::vector<double>(lig_nmodes, lig_nmodes + lig_nmodes_len));
        backbone_ = rec_.backbone;
        for (uint32_t a : lig_.backbone) backbone_.push_back(a + (uint32_t)d.n_rec);
        d_backbone_ = arena_.upload(backbone_);
        std::vector<uint32_t> res_start(rec_.res_start.begin(), rec_.res_start.end() - 1);
        for (uint32_t a : lig_.res_start) res_start.push_back(a + (uint32_t)d.n_rec);
        ContactsDevice &k = contacts_;
        k.n_atoms = d.n_rec + d.n_lig;
        k.n_rec_res = (int)rec_.res_id.size();
        k.n_lig_res = (int)lig_.res_id.size();
        k.n_lig_grp = (k.n_lig_res + kResGroup - 1) / kResGroup;
        k.res_start = arena_.upload(res_start);
        std::vector<uint32_t> res_of_atom = rec_.res_of_atom;
        for (uint32_t r : lig_.res_of_atom) res_of_atom.push_back(r + (uint32_t)k.n_rec_res);
        k.res_of_atom = arena_.upload(res_of_atom);
        k.boxes_in_lds = k.box_bytes() <= kMaxBoxLdsBytes;
        // the atoms that take part in the surface, the receptor's first
        std::vector<uint32_t> part_atom, part_radius;
        const PdbFile *files[2] = {&rec_, &lig_};
        for (int side = 0; side < 2; side++) {
            for (size_t a = 0; a < files[side]->lines.size(); a++) {
                const uint32_t r = sasa_radius(files[side]->lines[a].data(), files[side]->lines[a].size());
                sasa_radius_[side].push_back(r);
                if (r == 0) continue;
                part_atom.push_back((uint32_t)(side * rec_.lines.size() + a));
                part_radius.push_back(r);
                sasa_r_max_ = std::max(sasa_r_max_, (int)r);
            }
            if (side == 0) sasa_.n_part_rec = (int)part_atom.size();
        }
        sasa_.n_atoms = k.n_atoms;
        sasa_.n_part = (int)part_atom.size();
        sasa_.part_atom = arena_.upload(part_atom);
        sasa_.part_radius = arena_.upload(part_radius);
        init_saxs();
    } catch (...) {
        destroy();  // no destructor runs for a constructor that throws
        throw;
    }
}

void Complex::destroy() {
    // the buffers are freed after this: nothing queued (a call that threw halfway) may still use them
    if (stream_) (void)hipStreamSynchronize(stream_);
    if (ev0_) (void)hipEventDestroy(ev0_);
    if (ev1_) (void)hipEventDestroy(ev1_);
    if (stream_) (void)hipStreamDestroy(stream_);
}

const PdbFile &Complex::side_file(int side) const {
    if (side != 0 && side != 1) throw Error(LD_ERR_INVALID, "side must be 0 (receptor) or 1 (ligand)");
    return side == 0 ? rec_ : lig_;
}

void Complex::residue_id(int side, size_t index, char *buf, size_t buf_len) const {
    if (!buf) throw Error(LD_ERR_INVALID, "null argument");
    const std::vector<std::string> &ids = side_file(side).res_id;
    if (index >= ids.size()) throw Error(LD_ERR_INVALID, "residue index out of range");
    if (ids[index].size() + 1 > buf_len) throw Error(LD_ERR_INVALID, "buffer too short for the residue id");
    std::memcpy(buf, ids[index].c_str(), ids[index].size() + 1);
}

void Complex::residue_of_atom(int side, uint32_t *out) const {
    if (!out) throw Error(LD_ERR_INVALID, "null argument");
    const std::vector<uint32_t> &of = side_file(side).res_of_atom;
    std::copy(of.begin(), of.end(), out);
}

void Complex::check_poses(size_t n, const double *poses, size_t stride) const {
    const size_t len = pose_len();
    if (n && !poses) throw Error(LD_ERR_INVALID, "null poses");
    if (stride < len) throw Error(LD_ERR_INVALID, "pose stride below the pose length");
    for (size_t i = 0; i < n; i++) {
        const double *row = poses + i * stride;
        for (size_t k = 0; k < len; k++)
            if (!std::isfinite(row[k])) throw Error(LD_ERR_INVALID, "pose " + std::to_string(i) + " is not finite");
        if (row[3] == 0.0 && row[4] == 0.0 && row[5] == 0.0 && row[6] == 0.0)
            throw Error(LD_ERR_INVALID, "pose " + std::to_string(i) + " has a zero quaternion");
    }
}

void Complex::upload_poses(size_t n, const double *poses, size_t stride) {
    reserve_exact(d_poses_, n * stride * sizeof(double));
    hip_check(hipMemcpyAsync(d_poses_.ptr, poses, n * stride * sizeof(double), hipMemcpyHostToDevice, stream_), "hipMemcpy H2D poses");
}

void Complex::pose_all(size_t n, const double *poses, size_t stride, double *out) {
    const size_t per_pose = n_atoms() * 3 * sizeof(double);
    const size_t chunk = chunk_of(per_pose, n);
    upload_poses(n, poses, stride);
    for (size_t i0 = 0; i0 < n; i0 += chunk) {
        const size_t m = std::min(chunk, n - i0);
        reserve_exact(d_out_, m * per_pose);
        hip_check(launch_complex_pose_xyz(dev_, static_cast<const double *>(d_poses_.ptr) + i0 * stride, stride, m,
                                          static_cast<double *>(d_out_.ptr), stream_),
                  "complex_pose_xyz launch");
        hip_check(hipMemcpyAsync(out + i0 * n_atoms() * 3, d_out_.ptr, m * per_pose, hipMemcpyDeviceToHost, stream_),
                  "hipMemcpy D2H coordinates");
    }
    hip_check(hipStreamSynchronize(stream_), "complex_pose_xyz");
}

void Complex::coordinates(size_t n, const double *poses, size_t stride, double *xyz_out) {
    if (n && !xyz_out) throw Error(LD_ERR_INVALID, "null argument");
    check_poses(n, poses, stride);
    if (n) pose_all(n, poses, stride, xyz_out);
}

void Complex::begin_timed(int *d_overflow) {
    hip_check(hipMemsetAsync(d_overflow, 0, sizeof(int), stream_), "hipMemset");
    hip_check(hipEventRecord(ev0_, stream_), "hipEventRecord");
}

void Complex::finish_timed(const int *d_overflow, const char *what, const char *overflow_message) {
    hip_check(hipEventRecord(ev1_, stream_), "hipEventRecord");
    int overflow = 0;
    hip_check(hipMemcpyAsync(&overflow, d_overflow, sizeof(int), hipMemcpyDeviceToHost, stream_), "hipMemcpy D2H");
    hip_check(hipStreamSynchronize(stream_), what);
    if (overflow) throw Error(LD_ERR_INVALID, overflow_message);
    float ms = 0.0f;
    hip_check(hipEventElapsedTime(&ms, ev0_, ev1_), "hipEventElapsedTime");
    last_kernel_ms_ = ms;
}

void Complex::cluster(size_t n_swarms, size_t n_glowworms, const double *poses, size_t stride, const double *scoring, double cutoff,
                      int32_t *cluster_of, int32_t *representatives, uint32_t *n_clusters) {
    if (n_glowworms == 0 || n_glowworms > (size_t)kMaxGlowworms) throw Error(LD_ERR_INVALID, "n_glowworms must be 1 .. 4096");
    if (std::isnan(cutoff)) throw Error(LD_ERR_INVALID, "cutoff is NaN");
    if (backbone_.empty()) throw Error(LD_ERR_INVALID, "the complex has no atom named CA or P");
    if (n_swarms == 0) return;
    if (!scoring || !cluster_of || !representatives || !n_clusters) throw Error(LD_ERR_INVALID, "null argument");
    const size_t n = n_swarms * n_glowworms;
    check_poses(n, poses, stride);
    check_scoring(n, scoring);

    const int G = (int)n_glowworms, n_bb = (int)backbone_.size();
    const size_t per_swarm = (size_t)G * n_bb * 3 * sizeof(int32_t);
    const size_t chunk = chunk_of(per_swarm, n_swarms);
    upload_poses(n, poses, stride);
    reserve_exact(d_scores_, n * sizeof(double));
    hip_check(hipMemcpyAsync(d_scores_.ptr, scoring, n * sizeof(double), hipMemcpyHostToDevice, stream_), "hipMemcpy H2D scoring");
    int32_t *d_cluster, *d_reps;
    uint32_t *d_count;
    int *d_overflow;
    carve_into(d_ids_, [&](Carver &c) {
        d_cluster = c.take<int32_t>(n), d_reps = c.take<int32_t>(n);
        d_count = c.take<uint32_t>(n_swarms), d_overflow = c.take<int>(1);
    });
    reserve_exact(d_ws_, chunk * per_swarm);
    int32_t *d_ws = static_cast<int32_t *>(d_ws_.ptr);
    const double *d_poses = static_cast<const double *>(d_poses_.ptr);
    const double *d_scores = static_cast<const double *>(d_scores_.ptr);
    begin_timed(d_overflow);
    for (size_t s0 = 0; s0 < n_swarms; s0 += chunk) {
        const int m = (int)std::min(chunk, n_swarms - s0);
        hip_check(launch_complex_pose_thousandths(dev_, d_poses + s0 * G * stride, stride, m, G, d_backbone_, n_bb, d_ws, d_overflow,
                                                  stream_),
                  "complex_pose_thousandths launch");
        hip_check(launch_complex_bsas(d_ws, d_scores + s0 * G, m, G, n_bb, cutoff, d_cluster + s0 * G, d_reps + s0 * G, d_count + s0,
                                      stream_),
                  "complex_bsas launch");
    }
    finish_timed(d_overflow, "complex_bsas", "a posed backbone coordinate is beyond +-2.1e6 A");
    hip_check(hipMemcpy(cluster_of, d_cluster, n * sizeof(int32_t), hipMemcpyDeviceToHost), "hipMemcpy D2H");
    hip_check(hipMemcpy(representatives, d_reps, n * sizeof(int32_t), hipMemcpyDeviceToHost), "hipMemcpy D2H");
    hip_check(hipMemcpy(n_clusters, d_count, n_swarms * sizeof(uint32_t), hipMemcpyDeviceToHost), "hipMemcpy D2H");
}

void Complex::cluster_ranked(size_t n, const double *poses, size_t stride, const double *scoring, double cutoff, int atoms,
                             int32_t *cluster_of, int32_t *representatives, uint32_t *n_clusters) {
    if (std::isnan(cutoff)) throw Error(LD_ERR_INVALID, "cutoff is NaN");
    if (atoms != 0 && atoms != 1) throw Error(LD_ERR_INVALID, "atoms must be 0 (the complex's CA / P atoms) or 1 (the ligand's)");
    if (!n_clusters) throw Error(LD_ERR_INVALID, "null argument");
    // the walk: the ligand's CA / P atoms first, they move most.  Without receptor modes the receptor's terms are zero
    // and are not walked; the RMSD still counts them.
    std::vector<uint32_t> walk;
    for (uint32_t a : lig_.backbone) walk.push_back(a + (uint32_t)dev_.n_rec);
    const size_t measured = atoms == 1 ? walk.size() : backbone_.size();
    if (measured == 0)
        throw Error(LD_ERR_INVALID, atoms == 1 ? "the ligand has no atom named CA or P" : "the complex has no atom named CA or P");
    if (atoms == 0 && (dev_.anm_rec > 0 || walk.empty())) walk.insert(walk.end(), rec_.backbone.begin(), rec_.backbone.end());
    // the bound comes before anything reads the list
    const size_t per_pose = walk.size() * 3 * sizeof(int32_t);
    if (n > kRankedWorkspaceBytes / per_pose)
        throw Error(LD_ERR_INVALID, "the list's workspace (" + std::to_string(per_pose) + " B a pose) would exceed 4 GiB");
    if (n == 0) {
        *n_clusters = 0;
        return;
    }
    if (!scoring || !cluster_of || !representatives) throw Error(LD_ERR_INVALID, "null argument");
    check_poses(n, poses, stride);
    check_scoring(n, scoring);

    // (scoring descending, index ascending); everything on the device is indexed by sorted position
    std::vector<int32_t> order(n);
    for (size_t i = 0; i < n; i++) order[i] = (int32_t)i;
    std::stable_sort(order.begin(), order.end(), [scoring](int32_t a, int32_t b) { return scoring[a] > scoring[b]; });
    const size_t len = pose_len();
    std::vector<double> sorted(n * len);
    for (size_t p = 0; p < n; p++) std::copy(poses + (size_t)order[p] * stride, poses + (size_t)order[p] * stride + len, &sorted[p * len]);

    upload_poses(n, sorted.data(), len);
    RankedStatus *d_status;
    uint32_t *d_walk;
    RankedLaunch r;
    r.n = (int)n;
    r.n_walk = (int)walk.size();
    carve_into(d_ids_, [&](Carver &c) {
        r.status = d_status = c.take<RankedStatus>(1), d_walk = c.take<uint32_t>(walk.size());
        r.state = c.take<int32_t>(2 * n);  // one array: the ids, then the leaders
    });
    r.reps = r.state + n;
    reserve_exact(d_ranked_ws_, n * per_pose);
    int32_t *d_ws = static_cast<int32_t *>(d_ranked_ws_.ptr);
    hip_check(hipMemcpyAsync(d_walk, walk.data(), walk.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream_), "hipMemcpy H2D walk");
    hip_check(hipEventRecord(ev0_, stream_), "hipEventRecord");
    hip_check(launch_ranked_begin(r, cutoff, (double)measured, stream_), "ranked_begin launch");
    hip_check(launch_ranked_pose(dev_, static_cast<const double *>(d_poses_.ptr), len, r.n, d_walk, r.n_walk, d_ws, d_status, stream_),
              "ranked_pose launch");
    // a round: the pick's candidates, then the sweep behind them (sized from the cursor BEFORE the pick, which the sweep
    // corrects from the status); the host reads the status once a round.  Every round resolves a candidate or ends the loop.
    const char *beyond = "a posed CA / P coordinate is beyond +-2.1e6 A";
    RankedStatus st;
    int from = 0;
    for (;;) {
        hip_check(launch_ranked_pick(r, d_ws, stream_), "ranked_pick launch");
        hip_check(launch_ranked_sweep(r, d_ws, from, stream_), "ranked_sweep launch");
        hip_check(hipMemcpyAsync(&st, d_status, sizeof st, hipMemcpyDeviceToHost, stream_), "hipMemcpy D2H status");
        hip_check(hipStreamSynchronize(stream_), "ranked round");
        if (st.overflow) throw Error(LD_ERR_INVALID, beyond);
        if (st.n_candidates == 0) break;
        if (st.cursor <= from || st.cursor > r.n) throw Error(LD_ERR_DEVICE, "ranked clustering: the cursor did not advance");
        from = st.cursor;
    }
    finish_timed(&d_status->overflow, "ranked clustering", beyond);
    const size_t k = (size_t)st.n_clusters;
    std::vector<int32_t> state(n), reps(k);
    hip_check(hipMemcpy(state.data(), r.state, n * sizeof(int32_t), hipMemcpyDeviceToHost), "hipMemcpy D2H");
    hip_check(hipMemcpy(reps.data(), r.reps, k * sizeof(int32_t), hipMemcpyDeviceToHost), "hipMemcpy D2H");
    for (size_t p = 0; p < n; p++) cluster_of[order[p]] = state[p];
    for (size_t c = 0; c < n; c++) representatives[c] = c < k ? order[reps[c]] : -1;
    *n_clusters = (uint32_t)k;
}

void Complex::contacts(size_t n, const double *poses, size_t stride, double cutoff, uint32_t *rec_bits, uint32_t *lig_bits) {
    const long long C = cutoff_thousandths(cutoff, "cutoff must be 0.001 .. 30 A");
    if (n == 0) return;
    check_poses(n, poses, stride);
    const ContactsDevice &k = contacts_;
    const size_t rw = ((size_t)k.n_rec_res + 31) / 32, lw = ((size_t)k.n_lig_res + 31) / 32;
    if (rw + lw > kMaxContactWords) throw Error(LD_ERR_INVALID, "more than 524288 residues");
    // a workspace slot a workgroup in flight: the atoms, and the boxes when LDS does not hold them
    const size_t per_slot = (size_t)k.n_atoms * sizeof(int4) + (k.boxes_in_lds ? 0 : k.box_bytes());
    const size_t slots = chunk_of(per_slot, n, kContactSlots);
    upload_poses(n, poses, stride);
    uint32_t *d_rec, *d_lig;
    int *d_overflow, *d_boxes;
    int4 *d_atoms;
    carve_into(d_ids_, [&](Carver &c) { d_rec = c.take<uint32_t>(n * rw), d_lig = c.take<uint32_t>(n * lw), d_overflow = c.take<int>(1); });
    carve_into(d_ws_, [&](Carver &c) {
        d_atoms = c.take<int4>(slots * k.n_atoms), d_boxes = c.take<int>(k.boxes_in_lds ? 0 : slots * 6 * (size_t)k.n_boxes());
    });
    begin_timed(d_overflow);
    hip_check(launch_complex_contacts(dev_, k, static_cast<const double *>(d_poses_.ptr), stride, n, (uint32_t)(C * C), slots, d_atoms,
                                      d_boxes, d_rec, d_lig, d_overflow, stream_),
              "complex_contacts launch");
    finish_timed(d_overflow, "complex_contacts", "a posed coordinate is beyond +-1.0e6 A");
    if (rec_bits) hip_check(hipMemcpy(rec_bits, d_rec, n * rw * sizeof(uint32_t), hipMemcpyDeviceToHost), "hipMemcpy D2H");
    if (lig_bits) hip_check(hipMemcpy(lig_bits, d_lig, n * lw * sizeof(uint32_t), hipMemcpyDeviceToHost), "hipMemcpy D2H");
}

// --- the solvent-accessible surface (lightdock_hip.h, "Solvent-accessible surface"; kernels/sasa.hpp) ------------------

void Complex::sasa_radii(int side, uint32_t *radii_out) const {
    side_file(side);
    if (!radii_out) throw Error(LD_ERR_INVALID, "null argument");
    std::copy(sasa_radius_[side].begin(), sasa_radius_[side].end(), radii_out);
}

void Complex::sasa(size_t n, const double *poses, size_t stride, double probe, uint64_t *sums, uint8_t *free_counts,
                   uint8_t *bound_counts) {
    if (!(probe >= 0.0 && probe <= 2.0)) throw Error(LD_ERR_INVALID, "probe must be 0 .. 2.0 A");
    if (sasa_.n_part_rec == 0 || sasa_.n_part == sasa_.n_part_rec)
        throw Error(LD_ERR_INVALID, "no atom of a side takes part in the surface (all hydrogens or membrane beads)");
    if (n == 0) return;
    check_poses(n, poses, stride);
    SasaDevice d = sasa_;
    d.probe = (int)std::llrint(1000.0 * probe);
    d.e_max = sasa_r_max_ + d.probe;
    const bool atoms = free_counts || bound_counts;
    const size_t n_all = n_atoms(), per_slot = sasa_slot_bytes(d.n_part);
    const size_t slots = chunk_of(per_slot, n, kSasaSlots);
    // per-atom counts leave in chunks of poses; nothing reaches the caller before the overflow flag is known
    const size_t chunk = atoms ? chunk_of(2 * n_all, n) : n, counts = atoms ? chunk * n_all : 0;
    std::vector<uint8_t> h_free(atoms ? n * n_all : 0), h_bound(atoms ? n * n_all : 0);
    upload_poses(n, poses, stride);
    unsigned long long *d_sums;
    int *d_overflow;
    uint8_t *d_free, *d_bound;  // null without `atoms`
    carve_into(d_ids_, [&](Carver &c) {
        d_sums = c.take<unsigned long long>(n * 4), d_overflow = c.take<int>(1);
        d_free = c.take<uint8_t>(counts), d_bound = c.take<uint8_t>(counts);
    });
    reserve_exact(d_ws_, slots * per_slot);  // launch_complex_sasa lays out its slots itself
    const double *d_poses = static_cast<const double *>(d_poses_.ptr);
    begin_timed(d_overflow);
    for (size_t i0 = 0; i0 < n; i0 += chunk) {
        const size_t m = std::min(chunk, n - i0);
        if (atoms) {  // atoms that take no part stay 0; each array by itself: the padding between two is nobody's
            hip_check(hipMemsetAsync(d_free, 0, counts, stream_), "hipMemset");
            hip_check(hipMemsetAsync(d_bound, 0, counts, stream_), "hipMemset");
        }
        hip_check(launch_complex_sasa(dev_, d, d_poses + i0 * stride, stride, m, std::min(slots, m), d_ws_.ptr, d_sums + i0 * 4, d_free,
                                      d_bound, d_overflow, stream_),
                  "complex_sasa launch");
        if (atoms) {
            hip_check(hipMemcpyAsync(h_free.data() + i0 * n_all, d_free, m * n_all, hipMemcpyDeviceToHost, stream_), "hipMemcpy D2H");
            hip_check(hipMemcpyAsync(h_bound.data() + i0 * n_all, d_bound, m * n_all, hipMemcpyDeviceToHost, stream_), "hipMemcpy D2H");
        }
    }
    finish_timed(d_overflow, "complex_sasa", "a posed coordinate is beyond +-1.0e6 A");
    if (sums) hip_check(hipMemcpy(sums, d_sums, n * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost), "hipMemcpy D2H");
    if (free_counts) std::copy(h_free.begin(), h_free.end(), free_counts);
    if (bound_counts) std::copy(h_bound.begin(), h_bound.end(), bound_counts);
}

// --- model quality against a reference complex (lightdock_hip.h, "Model quality"; kernels/assess.hpp) ------------------

namespace {

std::string trimmed_field(const std::string &line, size_t pos, size_t len) {
    const std::string s = line.substr(pos, len);
    const size_t b = s.find_first_not_of(' ');
    return b == std::string::npos ? std::string() : s.substr(b, s.find_last_not_of(' ') - b + 1);
}

// chain, sequence number, insertion code, residue name, atom name: columns 22, 23-26, 27, 18-20, 13-16, blanks trimmed
std::string record_key(const std::string &line) {
    return trimmed_field(line, 21, 1) + '\n' + trimmed_field(line, 22, 4) + '\n' + trimmed_field(line, 26, 1) + '\n' +
           trimmed_field(line, 17, 3) + '\n' + trimmed_field(line, 12, 4);
}

bool fit_name(const std::string &line) {
    const std::string name = trimmed_field(line, 12, 4);
    return name == "N" || name == "CA" || name == "C" || name == "O" || name == "P";
}

// For every record of `model` the first record of `reference` with the same key, or -1.
std::vector<int> match_records(const PdbFile &model, const PdbFile &reference) {
    std::map<std::string, int> first;
    for (size_t a = 0; a < reference.lines.size(); a++) first.emplace(record_key(reference.lines[a]), (int)a);
    std::vector<int> of(model.lines.size(), -1);
    for (size_t a = 0; a < model.lines.size(); a++) {
        const auto it = first.find(record_key(model.lines[a]));
        if (it != first.end()) of[a] = it->second;
    }
    return of;
}

struct RefSums {  // of a set of reference points, exact
    long long n = 0, s[3] = {};
    assess_wide ss = 0;
    void add(const long long r[3]) {
        n++;
        for (int k = 0; k < 3; k++) s[k] += r[k], ss += (assess_wide)r[k] * r[k];
    }
};

template <typename T>
const T *upload_into(DeviceBuffer &buffer, const std::vector<T> &host) {
    reserve_exact(buffer, std::max<size_t>(1, host.size()) * sizeof(T));
    if (!host.empty()) hip_check(hipMemcpy(buffer.ptr, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy H2D");
    return static_cast<const T *>(buffer.ptr);
}

}  // namespace

void Complex::set_reference(const char *ref_receptor_pdb, const char *ref_ligand_pdb, double contact_cutoff, double interface_cutoff) {
    if (stream_) hip_check(hipStreamSynchronize(stream_), "hipStreamSynchronize");  // nothing queued reads the old reference
    ref_ = Reference();  // a refusal below leaves the complex without a reference
    const long long C = cutoff_thousandths(contact_cutoff, "contact_cutoff must be 0.001 .. 30 A");
    const long long I = cutoff_thousandths(interface_cutoff, "interface_cutoff must be 0.001 .. 30 A");
    const PdbFile ref[2] = {read_pdb_file_order(ref_receptor_pdb), read_pdb_file_order(ref_ligand_pdb)};
    const PdbFile *model[2] = {&rec_, &lig_};
    const size_t n_rec = rec_.lines.size();

    // matching; the reference's thousandths of every matched model atom (complex atom index)
    std::vector<int> matched[2] = {match_records(rec_, ref[0]), match_records(lig_, ref[1])};
    std::vector<long long> xyz(n_atoms() * 3, 0);
    std::vector<uint8_t> is_matched(n_atoms(), 0), is_fit(n_atoms(), 0);
    Reference r;
    for (int side = 0; side < 2; side++)
        for (size_t a = 0; a < matched[side].size(); a++) {
            if (matched[side][a] < 0) continue;
            const size_t atom = side * n_rec + a;
            for (int k = 0; k < 3; k++) xyz[3 * atom + k] = std::llrint(ref[side].xyz[3 * (size_t)matched[side][a] + k] * 1000.0);
            is_matched[atom] = 1;
            is_fit[atom] = fit_name(model[side]->lines[a]);
            r.counts[side]++;
            r.counts[3 + side] += is_fit[atom];
        }
    if (r.counts[3] < 3) throw Error(LD_ERR_INVALID, "fewer than 3 receptor fit atoms (matched N, CA, C, O, P) in the reference");
    if (r.counts[4] < 1) throw Error(LD_ERR_INVALID, "no ligand fit atom (matched N, CA, C, O, P) in the reference");

    // native residue pairs and interface residues, on the reference's exact integers
    const size_t n_rec_res = rec_.res_id.size(), n_lig_res = lig_.res_id.size();
    std::vector<uint64_t> pairs;
    std::vector<uint8_t> interface_res[2] = {std::vector<uint8_t>(n_rec_res, 0), std::vector<uint8_t>(n_lig_res, 0)};
    std::vector<uint32_t> lig_atoms;
    for (size_t b = 0; b < lig_.lines.size(); b++)
        if (is_matched[n_rec + b]) lig_atoms.push_back((uint32_t)b);
    for (size_t a = 0; a < n_rec; a++) {
        if (!is_matched[a]) continue;
        const long long *p = &xyz[3 * a];
        const uint32_t ra = rec_.res_of_atom[a];
        for (uint32_t b : lig_atoms) {
            const long long *q = &xyz[3 * (n_rec + b)];
            const long long dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
            if (std::llabs(dx) > 30000 || std::llabs(dy) > 30000 || std::llabs(dz) > 30000) continue;
            const long long d2 = dx * dx + dy * dy + dz * dz;
            const uint32_t rb = lig_.res_of_atom[b];
            if (d2 <= I * I) interface_res[0][ra] = interface_res[1][rb] = 1;
            if (d2 <= C * C) pairs.push_back((uint64_t)ra << 32 | rb);
        }
    }
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    if (pairs.empty()) throw Error(LD_ERR_INVALID, "no native residue pair within contact_cutoff in the reference");
    if (pairs.size() > (size_t)INT32_MAX) throw Error(LD_ERR_INVALID, "too many native residue pairs");
    std::vector<uint8_t> native_res[2] = {std::vector<uint8_t>(n_rec_res, 0), std::vector<uint8_t>(n_lig_res, 0)};
    for (uint64_t p : pairs) {
        native_res[0][p >> 32] = native_res[1][(uint32_t)p] = 1;
        r.native.push_back((uint32_t)(p >> 32));
        r.native.push_back((uint32_t)p);
    }
    r.counts[2] = (uint32_t)pairs.size();

    // the centre: the integer-rounded centroid of the reference's receptor fit atoms
    long long centre[3] = {0, 0, 0};
    for (size_t a = 0; a < n_rec; a++)
        if (is_fit[a])
            for (int k = 0; k < 3; k++) centre[k] += xyz[3 * a + k];
    for (int k = 0; k < 3; k++) centre[k] = std::llrint((double)centre[k] / (double)r.counts[3]);

    // used atoms in index order: fit atoms and the matched atoms of the residues of a native pair
    std::vector<uint32_t> used_atom;
    std::vector<int4> used_ref;
    std::vector<int> lo[2] = {std::vector<int>(n_rec_res, 0), std::vector<int>(n_lig_res, 0)}, hi[2] = {lo[0], lo[1]};
    RefSums sums_rec, sums_lig, sums_int;
    for (size_t atom = 0; atom < n_atoms(); atom++) {
        const int side = atom >= n_rec;
        const uint32_t res = side ? lig_.res_of_atom[atom - n_rec] : rec_.res_of_atom[atom];
        if (atom == n_rec) r.dev.n_used_rec = (int)used_atom.size();
        if (!is_matched[atom] || !(is_fit[atom] || native_res[side][res])) continue;
        long long c[3];
        for (int k = 0; k < 3; k++) {
            c[k] = xyz[3 * atom + k] - centre[k];
            if (std::llabs(c[k]) > kAssessBound)
                throw Error(LD_ERR_INVALID, "a reference atom is more than 2000 A from the centroid of the receptor's fit atoms");
        }
        const int interface_fit = is_fit[atom] && interface_res[side][res];
        const int u = (int)used_atom.size();
        if (native_res[side][res]) {
            if (hi[side][res] == 0) lo[side][res] = u;
            hi[side][res] = u + 1;
        }
        used_atom.push_back((uint32_t)atom);
        used_ref.push_back(make_int4((int)c[0], (int)c[1], (int)c[2], (int)is_fit[atom] | interface_fit << 1));
        if (is_fit[atom]) (side ? sums_lig : sums_rec).add(c);
        if (interface_fit) sums_int.add(c);
    }
    if (n_rec == n_atoms()) r.dev.n_used_rec = (int)used_atom.size();
    r.counts[5] = (uint32_t)sums_int.n;
    if (sums_int.n < 3) throw Error(LD_ERR_INVALID, "fewer than 3 interface fit atoms within interface_cutoff in the reference");
    if (used_atom.size() > kAssessMaxUsed) throw Error(LD_ERR_INVALID, "more than 1048576 atoms to assess");
    std::vector<int4> native;
    for (uint64_t p : pairs) {
        const uint32_t i = (uint32_t)(p >> 32), j = (uint32_t)p;
        native.push_back(make_int4(lo[0][i], hi[0][i], lo[1][j], hi[1][j]));
    }

    // what the reference contributes to every pose's superpositions, exactly
    AssessSolve &k = r.solve;
    auto own = [](const RefSums &s) { return assess_to_double((assess_wide)s.n * s.ss - ((assess_wide)s.s[0] * s.s[0] + (assess_wide)s.s[1] * s.s[1] + (assess_wide)s.s[2] * s.s[2])) / (double)s.n; };
    k.n_rec = sums_rec.n, k.n_lig = sums_lig.n, k.n_int = sums_int.n;
    for (int a = 0; a < 3; a++) k.sr_rec[a] = sums_rec.s[a], k.sr_lig[a] = sums_lig.s[a], k.sr_int[a] = sums_int.s[a];
    k.g_rec = own(sums_rec);
    k.g_int = own(sums_int);
    {
        const assess_wide nr = sums_rec.n, nl = sums_lig.n;
        assess_wide dot = 0, rr = 0;
        for (int a = 0; a < 3; a++) dot += (assess_wide)sums_rec.s[a] * sums_lig.s[a], rr += (assess_wide)sums_rec.s[a] * sums_rec.s[a];
        k.g_lig = assess_to_double(nr * nr * sums_lig.ss - 2 * nr * dot + nl * rr) / ((double)sums_rec.n * (double)sums_rec.n);
    }

    r.C2 = (uint32_t)(C * C);
    r.dev.n_used = (int)used_atom.size();
    r.dev.n_native = (int)native.size();
    r.dev.used_atom = upload_into(d_ref_atoms_, used_atom);
    r.dev.used_ref = upload_into(d_ref_xyz_, used_ref);
    r.dev.native = upload_into(d_ref_native_, native);
    r.set = true;
    ref_ = std::move(r);
}

void Complex::reference_counts(uint32_t *out) const {
    if (!out) throw Error(LD_ERR_INVALID, "null argument");
    if (!ref_.set) throw Error(LD_ERR_INVALID, "no reference set (ld_complex_set_reference)");
    std::copy(ref_.counts, ref_.counts + 6, out);
}

void Complex::native_pairs(uint32_t *pairs) const {
    if (!pairs) throw Error(LD_ERR_INVALID, "null argument");
    if (!ref_.set) throw Error(LD_ERR_INVALID, "no reference set (ld_complex_set_reference)");
    std::copy(ref_.native.begin(), ref_.native.end(), pairs);
}

void Complex::assess(size_t n, const double *poses, size_t stride, uint32_t *kept, double *lrmsd, double *irmsd) {
    if (!ref_.set) throw Error(LD_ERR_INVALID, "no reference set (ld_complex_set_reference)");
    if (n == 0) return;
    check_poses(n, poses, stride);
    const AssessDevice &d = ref_.dev;
    // a chunk of poses a launch pair: its sums, and a workspace slot of used atoms a workgroup in flight
    const size_t chunk = std::min(n, kAssessChunkPoses);
    const size_t sums_bytes = chunk * kAssessWords * sizeof(long long), per_slot = (size_t)d.n_used * sizeof(int4);
    const size_t slots = chunk_of(per_slot, chunk, kAssessSlots, kClusterWorkspaceBytes - sums_bytes);
    upload_poses(n, poses, stride);
    double *d_lrmsd, *d_irmsd;
    uint32_t *d_kept;
    int *d_overflow;
    int4 *d_atoms;
    long long *d_sums;
    carve_into(d_ids_, [&](Carver &c) {
        d_lrmsd = c.take<double>(n), d_irmsd = c.take<double>(n), d_kept = c.take<uint32_t>(n), d_overflow = c.take<int>(1);
    });
    carve_into(d_ws_, [&](Carver &c) { d_atoms = c.take<int4>(slots * d.n_used), d_sums = c.take<long long>(chunk * kAssessWords); });
    const double *d_poses = static_cast<const double *>(d_poses_.ptr);
    begin_timed(d_overflow);
    for (size_t i0 = 0; i0 < n; i0 += chunk) {
        const size_t m = std::min(chunk, n - i0);
        hip_check(launch_complex_assess_sums(dev_, d, d_poses + i0 * stride, stride, m, ref_.C2, std::min(slots, m), d_atoms, d_sums,
                                             d_overflow, stream_),
                  "complex_assess_sums launch");
        hip_check(launch_complex_assess_solve(ref_.solve, d_sums, m, d_kept + i0, d_lrmsd + i0, d_irmsd + i0, stream_),
                  "complex_assess_solve launch");
    }
    finish_timed(d_overflow, "complex_assess", "a posed coordinate of an assessed atom is beyond +-2000 A");
    if (kept) hip_check(hipMemcpy(kept, d_kept, n * sizeof(uint32_t), hipMemcpyDeviceToHost), "hipMemcpy D2H");
    if (lrmsd) hip_check(hipMemcpy(lrmsd, d_lrmsd, n * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy D2H");
    if (irmsd) hip_check(hipMemcpy(irmsd, d_irmsd, n * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy D2H");
}

void Complex::write_pdb(const double *pose, const char *path) {
    if (!pose || !path) throw Error(LD_ERR_INVALID, "null argument");
    check_poses(1, pose, pose_len());
    std::vector<double> xyz(n_atoms() * 3);
    pose_all(1, pose, pose_len(), xyz.data());
    std::string text;
    text.reserve(n_atoms() * 82);
    char buf[32];
    size_t a = 0;
    for (const PdbFile *f : {&rec_, &lig_})
        for (const std::string &line : f->lines) {  // line[:30] + "%8.3f%8.3f%8.3f" + line[54:]
            std::snprintf(buf, sizeof buf, "%8.3f%8.3f%8.3f", xyz[3 * a], xyz[3 * a + 1], xyz[3 * a + 2]);
            text.append(line, 0, 30).append(buf).append(line, 54, std::string::npos).push_back('\n');
            a++;
        }
    std::FILE *out = std::fopen(path, "wb");
    if (!out) throw Error(LD_ERR_IO, std::string("cannot write ") + path);
    const bool ok = std::fwrite(text.data(), 1, text.size(), out) == text.size();
    if (std::fclose(out) != 0 || !ok) throw Error(LD_ERR_IO, std::string("cannot write ") + path);
}

}  // namespace ld
