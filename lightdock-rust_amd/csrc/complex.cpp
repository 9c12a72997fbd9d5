// complex.cpp -- the host side of the analysis half of a run: argument checks, workspace sizing and chunking, the launch
// sequences of kernels/cluster.hpp, and ld_complex_write_pdb's text.
#include "complex.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace ld {

namespace {

void check_modes(const char *side, const double *modes, size_t len, size_t num_anm, size_t n_atoms) {
    if (len != num_anm * n_atoms * 3 || (len && !modes))
        throw Error(LD_ERR_INVALID, std::string(side) + ": " + std::to_string(len) +
                                        " mode values, expected num_anm x atoms x 3 = " + std::to_string(num_anm * n_atoms * 3));
}

}  // namespace

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
    d_poses_.reserve(n * stride * sizeof(double));
    hip_check(hipMemcpyAsync(d_poses_.ptr, poses, n * stride * sizeof(double), hipMemcpyHostToDevice, stream_), "hipMemcpy H2D poses");
}

void Complex::pose_all(size_t n, const double *poses, size_t stride, double *out) {
    const size_t per_pose = n_atoms() * 3 * sizeof(double);
    const size_t chunk = std::max<size_t>(1, kClusterWorkspaceBytes / per_pose);
    upload_poses(n, poses, stride);
    for (size_t i0 = 0; i0 < n; i0 += chunk) {
        const size_t m = std::min(chunk, n - i0);
        d_out_.reserve(m * per_pose);
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

// The end of a timed launch sequence (ev0_ was recorded in front of it): the overflow flag, the synchronisation, the time.
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
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(scoring[i])) throw Error(LD_ERR_INVALID, "scoring " + std::to_string(i) + " is not finite");

    const int G = (int)n_glowworms, n_bb = (int)backbone_.size();
    const size_t per_swarm = (size_t)G * n_bb * 3 * sizeof(int32_t);
    const size_t chunk = std::max<size_t>(1, kClusterWorkspaceBytes / per_swarm);
    upload_poses(n, poses, stride);
    d_scores_.reserve(n * sizeof(double));
    hip_check(hipMemcpyAsync(d_scores_.ptr, scoring, n * sizeof(double), hipMemcpyHostToDevice, stream_), "hipMemcpy H2D scoring");
    d_ids_.reserve(2 * n * sizeof(int32_t) + n_swarms * sizeof(uint32_t) + sizeof(int));
    int32_t *d_cluster = static_cast<int32_t *>(d_ids_.ptr);
    int32_t *d_reps = d_cluster + n;
    uint32_t *d_count = reinterpret_cast<uint32_t *>(d_reps + n);
    int *d_overflow = reinterpret_cast<int *>(d_count + n_swarms);
    hip_check(hipMemsetAsync(d_overflow, 0, sizeof(int), stream_), "hipMemset");
    d_ws_.reserve(std::min(chunk, n_swarms) * per_swarm);
    int32_t *d_ws = static_cast<int32_t *>(d_ws_.ptr);
    const double *d_poses = static_cast<const double *>(d_poses_.ptr);
    const double *d_scores = static_cast<const double *>(d_scores_.ptr);
    hip_check(hipEventRecord(ev0_, stream_), "hipEventRecord");
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

void Complex::contacts(size_t n, const double *poses, size_t stride, double cutoff, uint32_t *rec_bits, uint32_t *lig_bits) {
    const double scaled = cutoff * 1000.0;
    if (!(scaled > 0.0 && scaled < 30001.0)) throw Error(LD_ERR_INVALID, "cutoff must be 0.001 .. 30 A");
    const long long C = std::llrint(scaled);
    if (C < 1 || C > 30000) throw Error(LD_ERR_INVALID, "cutoff must be 0.001 .. 30 A");
    if (n == 0) return;
    check_poses(n, poses, stride);
    const ContactsDevice &k = contacts_;
    const size_t rw = ((size_t)k.n_rec_res + 31) / 32, lw = ((size_t)k.n_lig_res + 31) / 32;
    if (rw + lw > kMaxContactWords) throw Error(LD_ERR_INVALID, "more than 524288 residues");
    // a workspace slot a workgroup in flight: the atoms, and the boxes when LDS does not hold them
    const size_t per_slot = (size_t)k.n_atoms * sizeof(int4) + (k.boxes_in_lds ? 0 : k.box_bytes());
    const size_t slots = std::min(n, std::min<size_t>(kContactSlots, std::max<size_t>(1, kClusterWorkspaceBytes / per_slot)));
    upload_poses(n, poses, stride);
    d_ids_.reserve(n * (rw + lw) * sizeof(uint32_t) + sizeof(int));
    uint32_t *d_rec = static_cast<uint32_t *>(d_ids_.ptr);
    uint32_t *d_lig = d_rec + n * rw;
    int *d_overflow = reinterpret_cast<int *>(d_lig + n * lw);
    hip_check(hipMemsetAsync(d_overflow, 0, sizeof(int), stream_), "hipMemset");
    d_ws_.reserve(slots * per_slot);
    int4 *d_atoms = static_cast<int4 *>(d_ws_.ptr);
    hip_check(hipEventRecord(ev0_, stream_), "hipEventRecord");
    hip_check(launch_complex_contacts(dev_, k, static_cast<const double *>(d_poses_.ptr), stride, n, (uint32_t)(C * C), slots, d_atoms,
                                      reinterpret_cast<int *>(d_atoms + slots * k.n_atoms), d_rec, d_lig, d_overflow, stream_),
              "complex_contacts launch");
    finish_timed(d_overflow, "complex_contacts", "a posed coordinate is beyond +-1.0e6 A");
    if (rec_bits) hip_check(hipMemcpy(rec_bits, d_rec, n * rw * sizeof(uint32_t), hipMemcpyDeviceToHost), "hipMemcpy D2H");
    if (lig_bits) hip_check(hipMemcpy(lig_bits, d_lig, n * lw * sizeof(uint32_t), hipMemcpyDeviceToHost), "hipMemcpy D2H");
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
