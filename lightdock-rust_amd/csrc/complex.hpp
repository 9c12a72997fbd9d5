// complex.hpp -- the object behind an `ld_complex*`: a receptor and a ligand as their PDB files give them, device-resident,
// and the workspace of the analysis kernels (kernels/cluster.hpp).  What lightdock_hip.h says of ld_complex_*
// holds for the methods of the same names; refusals are ld::Error.  Every block that holds more than one array is laid out
// once, through device_memory.hpp's Carver (carve_into); a chunk or a slot count is chunk_of(); a timed launch sequence
// stands between begin_timed() and finish_timed().
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "device_memory.hpp"
#include "fcc.hpp"
#include "host/pdb_file.hpp"
#include "kernels/assess.hpp"
#include "kernels/cluster.hpp"
#include "kernels/ranked.hpp"
#include "kernels/sasa.hpp"
#include "kernels/saxs.hpp"

namespace ld {

class Density;

// C = llrint(cutoff * 1000), 1 .. 30000, of a contact cutoff in A (lightdock_hip.h, "Interface contacts"); `message` otherwise.
long long cutoff_thousandths(double cutoff, const char *message);
// The element of an ATOM / HETATM record: columns 77-78, trimmed and upper-cased; a record too short for them or a blank
// field: the first alphabetic character of columns 13-16.  `line` has 54 columns at least.
std::string record_element(const char *line, size_t len);
// The residue name of a record, columns 18-20, blanks trimmed.
std::string record_residue_name(const char *line);
// How many of n items of `per_item` bytes go at a time: what `budget` holds, one at least, n and `cap` at most.
inline size_t chunk_of(size_t per_item, size_t n, size_t cap = SIZE_MAX, size_t budget = kClusterWorkspaceBytes) {
    return std::min(std::min(n, cap), std::max<size_t>(1, budget / per_item));
}
// Refuses a scoring that is not finite.
void check_scoring(size_t n, const double *scoring);

class Complex {
   public:
    Complex(const char *receptor_pdb, const char *ligand_pdb, const double *rec_nmodes, size_t rec_nmodes_len, size_t rec_num_anm,
            const double *lig_nmodes, size_t lig_nmodes_len, size_t lig_num_anm);
    ~Complex() { destroy(); }
    Complex(const Complex &) = delete;
    Complex &operator=(const Complex &) = delete;

    size_t pose_len() const { return 7 + (size_t)dev_.anm_rec + (size_t)dev_.anm_lig; }
    size_t num_atoms(int side) const { return side == 0 ? rec_.lines.size() : side == 1 ? lig_.lines.size() : backbone_.size(); }
    size_t num_residues(int side) const { return side == 0 ? rec_.res_id.size() : side == 1 ? lig_.res_id.size() : 0; }
    void residue_id(int side, size_t index, char *buf, size_t buf_len) const;
    void residue_of_atom(int side, uint32_t *out) const;

    void coordinates(size_t n, const double *poses, size_t stride, double *xyz_out);
    void cluster(size_t n_swarms, size_t n_glowworms, const double *poses, size_t stride, const double *scoring, double cutoff,
                 int32_t *cluster_of, int32_t *representatives, uint32_t *n_clusters);
    // One ranked list across swarms (lightdock_hip.h, "Clustering a ranked list")
    void cluster_ranked(size_t n, const double *poses, size_t stride, const double *scoring, double cutoff, int atoms,
                        int32_t *cluster_of, int32_t *representatives, uint32_t *n_clusters);
    void contacts(size_t n, const double *poses, size_t stride, double cutoff, uint32_t *rec_bits, uint32_t *lig_bits);
    // Clustering by common contacts (lightdock_hip.h, "Clustering by common contacts"; fcc.cpp)
    void pair_contacts(size_t n, const double *poses, size_t stride, double cutoff, uint32_t *offsets, uint32_t *keys, size_t cap,
                       size_t *total_out);
    void cluster_fcc(size_t n, const double *poses, size_t stride, const double *scoring, double cutoff, double threshold,
                     uint32_t min_size, int32_t *cluster_of, int32_t *centres, uint32_t *n_clusters, uint32_t *set_sizes,
                     uint64_t *consensus);
    void write_pdb(const double *pose, const char *path);
    // Solvent-accessible surface (lightdock_hip.h, "Solvent-accessible surface")
    void sasa_radii(int side, uint32_t *radii_out) const;  // thousandths, 0 for an atom that takes no part
    void sasa(size_t n, const double *poses, size_t stride, double probe, uint64_t *sums, uint8_t *free_counts, uint8_t *bound_counts);
    // Collision cross-section (lightdock_hip.h, "Collision cross-section"; ccs.cpp)
    void ccs(size_t n, const double *poses, size_t stride, int what, double probe, double cell, uint32_t *counts, uint64_t *sums);
    // Cross-links (lightdock_hip.h, "Cross-links"; xlink.cpp)
    void crosslinks(size_t n, const double *poses, size_t stride, size_t n_links, const uint32_t *links, double probe, double cell,
                    double reach, double max_length, uint64_t *straight2, uint32_t *path);
    // Small-angle scattering (lightdock_hip.h, "Small-angle scattering"; saxs.cpp)
    void saxs_classes(int side, uint8_t *class_out) const;  // 0 .. 5, 255 for an atom that takes no part
    void saxs_chunk(size_t poses) { saxs_chunk_ = poses; }  // poses a chunk of counts; 0: as many as 256 MiB hold
    void distance_histogram(size_t n, const double *poses, size_t stride, uint32_t width, size_t bins, uint32_t *counts);
    void saxs(size_t n, const double *poses, size_t stride, uint32_t width, size_t bins, const double *q, size_t n_q, double *intensity,
              uint32_t *counts);
    // Density fit (lightdock_hip.h, "Density fit"; emfit.cpp)
    void density_chunk(size_t poses) { density_chunk_ = poses; }  // poses a chunk; 0: as many as 256 MiB hold
    void density_fit(Density &map, size_t n, const double *poses, size_t stride, uint32_t sigma, ld_density_sums *out);
    void simulate_density(Density &map, size_t n, const double *poses, size_t stride, uint32_t sigma, uint32_t *grid);
    // Model quality against a reference complex (lightdock_hip.h, "Model quality")
    void set_reference(const char *ref_receptor_pdb, const char *ref_ligand_pdb, double contact_cutoff, double interface_cutoff);
    void reference_counts(uint32_t *out) const;  // 6: matched rec, matched lig, native pairs, rec fit, lig fit, interface fit
    void native_pairs(uint32_t *pairs) const;    // n_native x 2
    void assess(size_t n, const double *poses, size_t stride, uint32_t *kept, double *lrmsd, double *irmsd);
    double last_kernel_ms() const { return last_kernel_ms_; }

   private:
    size_t n_atoms() const { return rec_.lines.size() + lig_.lines.size(); }
    const PdbFile &side_file(int side) const;
    void check_poses(size_t n, const double *poses, size_t stride) const;
    void upload_poses(size_t n, const double *poses, size_t stride);  // n rows of `stride` doubles, copied as they are
    void pose_all(size_t n, const double *poses, size_t stride, double *out);  // all atoms of n poses, unrounded
    // A timed launch sequence: after the uploads begin_timed clears the overflow word and records ev0_; finish_timed
    // records ev1_, reads the word, synchronises, refuses with `overflow_message` if it is set and keeps the time.
    void begin_timed(int *d_overflow);
    void finish_timed(const int *d_overflow, const char *what, const char *overflow_message);
    void check_pair_keys() const;
    void init_saxs();  // the atoms that take part in the scattering, from the constructor
    void saxs_run(size_t n, const double *poses, size_t stride, uint32_t width, size_t bins, const double *q, size_t n_q,
                  double *intensity, uint32_t *counts);
    void density_run(Density &map, size_t n, const double *poses, size_t stride, uint32_t sigma, ld_density_sums *out, uint32_t *grid);
    FccCluster::Sets pair_sets(size_t n, const double *poses, size_t stride, long long C, bool fill, size_t cap, int **d_overflow_out);
    void destroy();

    PdbFile rec_, lig_;
    std::vector<uint32_t> backbone_;  // complex atom indices: receptor CA / P, then ligand CA / P (offset by n_rec)
    DeviceArena arena_;
    ComplexDevice dev_;
    const uint32_t *d_backbone_ = nullptr;
    ContactsDevice contacts_;
    SasaDevice sasa_;                       // probe and e_max are set per call
    std::vector<uint32_t> sasa_radius_[2];  // every atom of a side, 0 for one that takes no part
    int sasa_r_max_ = 0;
    SaxsDevice saxs_;
    std::vector<uint8_t> saxs_class_[2];  // every atom of a side, 255 for one that takes no part
    uint32_t saxs_class_atoms_[kSaxsClasses] = {};
    size_t saxs_chunk_ = 0;
    size_t density_chunk_ = 0;
    DeviceBuffer d_density_;  // density_run's receptor grid and the voxels of a chunk
    DeviceBuffer d_ccs_;      // ccs's rigid receptor: its atoms, the layout and the bitmaps of its 64 views
    DeviceBuffer d_xlink_;    // crosslinks's links and their grouping by source anchor
    // what set_reference derived; `set` only once all of it stands
    struct Reference {
        bool set = false;
        uint32_t counts[6] = {};
        uint32_t C2 = 0;
        std::vector<uint32_t> native;  // (receptor residue, ligand residue), sorted
        AssessDevice dev;
        AssessSolve solve;
    } ref_;
    DeviceBuffer d_ref_atoms_, d_ref_xyz_, d_ref_native_;  // behind ref_.dev: a later reference reuses them
    // grow-only and shared by the methods; a call carves what it needs of d_out_, d_ws_ and d_ids_ anew (carve_into)
    DeviceBuffer d_poses_, d_scores_, d_out_, d_ws_, d_ids_;
    DeviceBuffer d_pair_keys_;  // the keys of pair_sets
    FccCluster fcc_;            // cluster_fcc's workspace
    DeviceBuffer d_ranked_ws_;  // cluster_ranked's resident thousandths (up to kRankedWorkspaceBytes), apart from d_ws_
    hipStream_t stream_ = nullptr;
    hipEvent_t ev0_ = nullptr, ev1_ = nullptr;
    double last_kernel_ms_ = 0.0;
};

}  // namespace ld

struct ld_complex {
    ld::Complex impl;
    ld_complex(const char *receptor_pdb, const char *ligand_pdb, const double *rec_nmodes, size_t rec_nmodes_len, size_t rec_num_anm,
               const double *lig_nmodes, size_t lig_nmodes_len, size_t lig_num_anm)
        : impl(receptor_pdb, ligand_pdb, rec_nmodes, rec_nmodes_len, rec_num_anm, lig_nmodes, lig_nmodes_len, lig_num_anm) {}
};
