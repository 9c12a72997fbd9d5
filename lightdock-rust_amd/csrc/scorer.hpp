// scorer.hpp -- the object behind an `ld_scorer*`: device-resident docking models + the
// workspace of the pose-energy kernels.  Plays the role of the reference's
// `Box<dyn Score>` (DFIRE / DNA structs, src/dfire.rs:193-198, src/dna.rs:367-372).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "decompose.hpp"
#include "device_memory.hpp"
#include "host/error.hpp"
#include "kernels/dfire_bm.hpp"
#include "kernels/dfire_packed.hpp"
#include "kernels/dfire_tiled.hpp"
#include "kernels/pose_energy.hpp"
#include "lightdock_hip.h"
#include "refine.hpp"

namespace ld {

struct HostMolecule {  // what ld_scorer_model_arrays hands back
    std::vector<double> coordinates;
    std::vector<uint32_t> dfire_types;
    std::vector<double> ele_charges, vdw_charges, vdw_radii;
};

// What the scorer knows of one molecule whichever route runs (slot_molecule: host arithmetic only).
struct SideFacts {
    int n = 0;                   // atoms
    int num_anm = 0;             // ANM modes a pose carries for this side: 0 unless the scorer uses ANM
    int flag_words = 0;          // uint32 words of interface flags per pose for this side
    std::vector<int32_t> slot;   // per original atom: its bit of the per-pose flag set, or -1
};

// DFIRE's distance binning as a lookup over cells of 0.25 A^2 (DESIGN.md "bin LUT").
int dfire_bin_reference(double dist2);               // the formula, src/dfire.rs:49-53,336-337
struct DfireBinning {
    std::vector<uint8_t> lut;   // kDfireLutCells: bin at the lower edge of each 0.25 A^2 cell
    std::vector<double> step;   // kDfireSteps: step[b] = first d2 the reference puts in bin >= b
};
DfireBinning build_dfire_binning();                  // throws if the self-check fails
double dfire_interface_d2();                         // largest d2 with sqrt(d2)*2-1 <= 3.9
std::vector<uint32_t> build_packed_lut(int cells_per_unit, double eps, uint32_t zero_bins = 0);  // kPackedLutCells * cells_per_unit words
size_t dfire_bm_reach_count(const double *xyz, size_t n, double reach);   // upper bound on the atoms inside any ball of that radius (n itself below 8192 atoms)
double dfire_bm_fix_scale(double vmax, size_t reach_count, int *extra_bits_out);   // the block-major path's fixed-point units per unit of the potential; 0.0: none fits
std::vector<uint8_t> build_bm_lut(double eps_cells, uint32_t zero_bins = 0);  // kBmLutBytes codes of the block-major kernel (kernels/dfire_bm.hpp)

struct TiledSoA {  // a molecule in tile order, SoA, padded to whole tiles
    int n_real = 0, n_tiles = 0;
    const double *x = nullptr, *y = nullptr, *z = nullptr;
    const uint32_t *tindex = nullptr;
    const int32_t *slot = nullptr;
    int num_anm = 0;
    const double *modes = nullptr;
    std::vector<double> hx, hy, hz;   // host copies, tile order (padding included)
    std::vector<uint32_t> htype;      // DFIRE type per slot of the tile order, 0xffffffff = padding
    std::vector<int32_t> hslot;       // interface-flag slot or -1
    std::vector<double> hmodes;       // host copy of `modes`: [mode][xyz][padded atoms]
};

struct ReceptorImage {  // the receptor as pair records and boxes in an f32 frame (dfire_packed_prepare's output)
    PackedRecPair *pairs = nullptr;
    TiledBox *sub = nullptr, *tile = nullptr;
};

// What the two culled DFIRE routes share (Scorer::build_tiles, before either route is chosen): both molecules in tile order,
// the ligand as the kernels read it, the potential in patches, and the bins no pair of this complex draws a value from.
struct DfireTiles {
    TiledSoA rec, lig;
    TiledLigand lig_view;              // `lig` as the culled kernels read it
    const double *table = nullptr;     // the potential in 2 x 2 x 4 patches (kernels/dfire_tiled.hpp)
    std::vector<uint32_t> type_perm_rec, type_perm_lig;  // DFIRE type -> number used by the patch table's layout
    uint32_t zero_bins = 0;            // bit b: the potential is zero in bin b for every type pair of the complex (LIGHTDOCK_PACKED_ELIDE_ZERO_BINS=0: none)
    // dfire_packed_prepare's arguments for the frame (centre, kappa, ubound): the receptor's; poses and outputs are the caller's
    PackedPrepareLaunch prepare(const double centre[3], double kappa, double ubound) const;
    // the undeformed receptor's image in that frame, in `arena`: one launch on `stream`, synchronised
    ReceptorImage static_image(DeviceArena &arena, const double centre[3], double kappa, double ubound, hipStream_t stream) const;
};

// What a culled route takes from the scorer that builds it.
struct RouteInputs {
    const ld_scorer_desc &desc;
    const DfireTiles &tiles;
    int rec_flag_words;
    const double *bin_step;   // kDfireSteps, d2 units (the scorer's upload, shared by every DFIRE route)
    double iface_d2;
    bool use_anm;
    bool latency;             // LIGHTDOCK_TILED_LATENCY: launches of one swarm
    int n_cus;
    hipStream_t stream;       // of the one launch a route's construction needs
};

// The per-pose buffers every route writes (the scorer's): one pose's partial sums, as many as the route leaves, and its flag words.
struct PoseOutputs {
    uint32_t *flags = nullptr;
    double *partial = nullptr;
    uint32_t *count_partial = nullptr, *tested_partial = nullptr, *exact_partial = nullptr;   // counting launches only
};

// ---------------------------------------------------------------------------------------
// The pose-major packed-f32 DFIRE route (kernels/dfire_packed.hpp) as one object
// ---------------------------------------------------------------------------------------
// What packed_accepts() derives of a receptor the route takes (host arithmetic only).
struct PackedFrame {
    double centre[3] = {0, 0, 0}, kappa = 2.0, ubound = 0.0, eps = 0.0;   // the record frame; the LUT's error bound (units of 4 d2)
    int cells = 1;                                                        // LUT cells per unit of 4 d2
};
bool packed_accepts(const ld_molecule &receptor, PackedFrame *out);   // false: the receptor is too long for the f32 frame (all pairs, f64)

class PackedPath {
   public:
    PackedPath(const RouteInputs &in, const PackedFrame &frame);
    // The largest batch run() takes: a receptor that flexes carries one image per pose, bounded to 8 GiB (LIGHTDOCK_RECEPTOR_IMAGE_MIB).
    size_t max_batch() const;
    // One batch: with a receptor that flexes dfire_packed_prepare, then dfire_packed_pairs, on `stream`.
    void run(size_t n, const double *d_poses, size_t stride, const uint8_t *d_active, const uint32_t *d_list, const uint32_t *d_count,
             const PoseOutputs &out, hipStream_t stream);
    uint64_t generation() const { return ws_rec_pairs_.generation + ws_rec_sub_.generation + ws_rec_tile_.generation; }
    size_t partials_per_pose() const { return (size_t)model_.n_groups * kPackedPartialsPerGroup; }
    const PackedLaunch &model() const { return model_; }

   private:
    const DfireTiles &tiles_;
    DeviceArena arena_;                           // the LUTs and a rigid receptor's image
    PackedLaunch model_;
    const uint32_t *lut_full_ = nullptr;          // the LUT without elided zero bins (counting launches)
    bool image_per_pose_ = false;                 // receptor ANM: one receptor image per pose per launch
    DeviceBuffer ws_rec_pairs_, ws_rec_sub_, ws_rec_tile_;
};

// ---------------------------------------------------------------------------------------
// The all-pairs route (kernels/pose_energy.hpp) as one object: DNA / PYDOCK, and DFIRE where no culled route runs
// ---------------------------------------------------------------------------------------
class AllPairsPath {
   public:
    // bin_step / iface_d2: the scorer's (bin_step is null for DNA)
    AllPairsPath(const ld_scorer_desc &desc, const SideFacts &rec, const SideFacts &lig, const double *bin_step, double iface_d2, int method,
                 bool use_anm);
    // One batch: pose_energy_pairs on `stream`, by the mask (d_list / d_count are not read).
    void run(size_t n, const double *d_poses, size_t stride, const uint8_t *d_active, const uint32_t *d_list, const uint32_t *d_count,
             const PoseOutputs &out, hipStream_t stream);
    size_t partials_per_pose() const { return (size_t)model_.n_chunks; }
    const PairLaunch &model() const { return model_; }

   private:
    DeviceMolecule upload_molecule(const ld_molecule &m, const SideFacts &facts, bool is_receptor);

    DeviceArena arena_;   // both molecules as the kernel reads them; DFIRE: the reference-layout potential and the cell LUT
    PairLaunch model_;    // molecule / table pointers and the chunking, filled once; batch fields per run()
};

// ---------------------------------------------------------------------------------------
// The block-major DFIRE route (kernels/dfire_bm.hpp) as one object
// ---------------------------------------------------------------------------------------
// The device buffers of kernels/dfire_bm.hpp's bm_layout(), grow-only.
struct BmWorkspace {
    DeviceBuffer buffer[kBmBuffers];
    void reserve(const BmLayout &layout) {
        for (int b = 0; b < kBmBuffers; b++) buffer[b].reserve(layout.buffer_bytes[b]);
    }
    uint64_t generation() const {
        uint64_t g = 0;
        for (const DeviceBuffer &b : buffer) g += b.generation;
        return g;
    }
    void point(BmLaunch &t, const BmLayout &layout, size_t set) const {
        void *ptrs[kBmBuffers];
        for (int b = 0; b < kBmBuffers; b++) ptrs[b] = buffer[b].ptr;
        bm_point_launch(t, layout, ptrs, set);
    }
};

// What bm_accepts() derives of a complex the path takes (host arithmetic only).
struct BmFrame {
    bool anm = false;
    double centre[3] = {0, 0, 0}, ubound = 0.0, extent = 0.0, eps = 0.0;   // the record frame; the LUT's error bound (cells)
    double sub_axis = 0.0, sub_diag = 0.0;         // the receptor's widest subtile box: half extent along an axis, half diagonal (record units)
    std::vector<float> tile_sphere, tile_radius;   // the ligand tiles' bounding spheres: [tile][4] as the culling kernel reads them; radii in angstrom (the reach of the fixed-point scale)
    double fix_scale = 0.0;
    size_t chunk = 0;                              // poses per pass
};
// the frame part of bm_accepts(): anm, centre, ubound, extent, eps of the two molecules' coordinates and the receptor's widest
// subtile box (dfire_bm_subtile_extents of its tile order; record units); false: eps reaches 8 cells
// kernels/dfire_bm.hpp's dfire_bm_error_bound(ubound, lig_extent, anm) with the widest receptor subtile box in it: its half extent
// along an axis and its half diagonal, record units (0, 0: nothing wider than the derivation assumes -- the three-argument form)
double dfire_bm_error_bound(double ubound, double lig_extent, bool anm, double sub_axis, double sub_diag);
void dfire_bm_subtile_extents(const std::vector<double> &x, const std::vector<double> &y, const std::vector<double> &z,
                              const std::vector<uint32_t> &type, double *sub_axis, double *sub_diag);
bool dfire_bm_frame(const ld_molecule &receptor, const ld_molecule &ligand, bool anm, double sub_axis, double sub_diag, BmFrame *out);

class BlockMajorPath {
   public:
    // nullptr: declined -- the complex stays with the pose-major kernels, and nothing was uploaded or launched for this path
    static std::unique_ptr<BlockMajorPath> build(const RouteInputs &in);
    ~BlockMajorPath();
    BlockMajorPath(const BlockMajorPath &) = delete;
    BlockMajorPath &operator=(const BlockMajorPath &) = delete;

    // the workspace of a batch of n poses (no allocation in a following run() of that size)
    void reserve(size_t n, bool counts) { ws_.reserve(bm_layout(shape(n, counts, false))); }
    // One batch: passes of at most pass_poses(n) poses, each dfire_bm_pose .. dfire_bm_gather, on `stream` (and, two passes in
    // flight, the path's second stream, joined before returning).  Leaves one partial per pose in `partial` and returns false:
    // pose_energy_finish is the caller's.  A batch of ONE pass that wants no pair counts (and no LIGHTDOCK_BM_DEBUG) ends in
    // dfire_bm_finish instead of dfire_bm_gather: the energies are written to `d_energies` with the scorer's `tail`, `partial`
    // is not, and run() returns true -- the step is one kernel shorter.  `pairs_done` (or nullptr) is then recorded in front of
    // dfire_bm_finish: the caller's timing brackets the pair kernels and not the tail, as it does around an unfused batch.
    bool run(size_t n, const double *d_poses, size_t stride, const uint8_t *d_active, const uint32_t *d_list, const uint32_t *d_count,
             const PoseOutputs &out, const TailTables &tail, double *d_energies, hipEvent_t pairs_done, hipStream_t stream);
    uint64_t generation() const { return ws_.generation(); }
    uint32_t quiet_subtiles() const { return quiet_subtiles_; }
    size_t pass_poses(size_t n) const;   // poses per pass of a batch of n
    size_t sets(size_t n) const;         // workspace sets a batch of n poses needs (2 while two passes are in flight)

   private:
    BlockMajorPath(const RouteInputs &in, const BmFrame &frame);
    BmShape shape(size_t n, bool counts, bool debug) const;

    DeviceArena arena_;                   // the model's uploads
    BmModel model_;
    size_t chunk_ = 0;                    // poses per pass (bounds the entry workspace)
    uint32_t quiet_subtiles_ = 0;         // receptor subtiles whose atoms' rows of the potential are zero
    int n_cus_ = 256;
    hipStream_t aux_stream_ = nullptr;    // the second of two passes in flight runs here
    hipEvent_t fork_ = nullptr, join_ = nullptr;
    BmWorkspace ws_;
};

class Scorer {
   public:
    explicit Scorer(const ld_scorer_desc &desc);
    ~Scorer();
    Scorer(const Scorer &) = delete;
    Scorer &operator=(const Scorer &) = delete;

    int method() const { return method_; }
    bool use_anm() const { return use_anm_; }
    size_t anm_rec() const { return (size_t)rec_.num_anm; }
    size_t anm_lig() const { return (size_t)lig_.num_anm; }
    size_t pose_len() const { return 7 + anm_rec() + anm_lig(); }
    size_t num_atoms(int side) const { return side ? (size_t)lig_.n : (size_t)rec_.n; }
    const HostMolecule &host_molecule(int side) const { return side ? host_lig_ : host_rec_; }
    int device() const { return device_; }
    hipStream_t stream() const { return stream_; }
    void set_stream(hipStream_t s) { stream_ = s ? s : own_stream_; }  // NULL: back to the handle's own stream
    void set_capturing(bool on) { capturing_ = on; }
    // make sure no allocation happens in the next energy_batch_device call of this size
    void prepare_batch(size_t n_poses) { reserve_workspace(n_poses, false); }
    // Changes whenever a workspace block of this scorer was reallocated (a larger batch came by): a
    // hipGraph captured before that replays kernels into freed memory and must be captured again.
    uint64_t workspace_generation() const;

    // Enqueue K1 for n poses already in HBM.  active / pair_counts may be null.  d_list / d_count
    // (device): the rows to evaluate as a compacted list whose length only the device knows (the GSO
    // loop: the glowworms that moved); they must be the rows `d_active` marks.
    void energy_batch_device(size_t n, const double *d_poses, size_t stride, const uint8_t *d_active,
                             double *d_energies, uint32_t *d_pair_counts, const uint32_t *d_list = nullptr,
                             const uint32_t *d_count = nullptr);
    // Host-pointer convenience: H2D, kernels, D2H, synchronise.
    void energy_batch_host(size_t n, const double *poses, size_t stride, double *energies);

    void kernel_info(ld_kernel_info *out) const;
    // diagnostics of the last counting launch: 8x8 atom-pair blocks evaluated per pose (culled DFIRE kernels)
    void last_block_counts(size_t n, uint32_t *out_host);
    uint32_t bm_quiet_subtiles() const { return bm_ ? bm_->quiet_subtiles() : 0u; }
    // how the block-major path would run a batch of n poses: poses per pass and workspace sets (0, 0 on the other routes)
    size_t bm_pass_poses(size_t n) const { return bm_ ? bm_->pass_poses(n) : 0; }
    size_t bm_sets(size_t n) const { return bm_ ? bm_->sets(n) : 0; }
    void enable_timing(bool on);
    void pair_kernel_time(double *total_ms, uint64_t *launches);

   private:
    void reserve_workspace(size_t n_poses, bool counts);
    size_t partials_per_pose() const;  // what the route that runs leaves for pose_energy_finish to fold
    void build_tiles(const ld_scorer_desc &desc);  // what the culled routes share (tiles_)
    void upload_tiled_molecule(const ld_molecule &m, bool is_receptor, TiledSoA &out, std::vector<uint32_t> &type_perm);

    int device_ = 0;
    hipStream_t stream_ = nullptr;
    hipStream_t own_stream_ = nullptr;
    bool capturing_ = false;
    int method_ = 0;
    bool use_anm_ = false;
    DeviceArena arena_;
    SideFacts rec_, lig_;
    TailTables tail_;
    // K1, fixed in the constructor: the block-major path (kernels/dfire_bm.hpp, the DFIRE default), the pose-major packed-f32
    // kernel (kernels/dfire_packed.hpp), or the all-pairs kernel of pose_energy.hpp (DNA, and DFIRE where the culled paths decline)
    enum class PairRoute { block_major, packed, all_pairs };
    PairRoute route_ = PairRoute::all_pairs;
    DfireTiles tiles_;                      // DFIRE unless LIGHTDOCK_DFIRE_KERNEL=allpairs; the routes below read it
    std::unique_ptr<BlockMajorPath> bm_;    // set: route_ == block_major
    std::unique_ptr<PackedPath> packed_;    // set: route_ == packed
    std::unique_ptr<AllPairsPath> all_pairs_;   // set: route_ == all_pairs
    int n_cus_ = 256;
    HostMolecule host_rec_, host_lig_;
    DeviceBuffer ws_partial_, ws_flags_, ws_counts_, ws_tested_, ws_exact_, ws_poses_, ws_energies_;
    bool timing_ = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events_;  // pool, reused
    size_t events_used_ = 0;
    double timed_ms_ = 0.0;
    uint64_t timed_launches_ = 0;
};

}  // namespace ld

struct ld_scorer {
    ld::Scorer impl;                               // checks the description before anything below reads it
    ld::DescCopy desc;                             // what the decomposer is built from, on first use
    std::unique_ptr<ld::Decomposer> decomposer;
    std::unique_ptr<ld::Refiner> refiner;          // ld_scorer_refine, on first use; runs its trial rows through `impl`
    explicit ld_scorer(const ld_scorer_desc &d) : impl(d), desc(d) {}
    ld::Decomposer &decompose() {
        if (!decomposer) decomposer.reset(new ld::Decomposer(desc.view()));
        return *decomposer;
    }
    ld::Refiner &refine() {
        if (!refiner) refiner.reset(new ld::Refiner(impl));
        return *refiner;
    }
};
