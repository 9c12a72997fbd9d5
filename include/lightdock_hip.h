/*
 * lightdock_hip.h -- C ABI of the MI355X (gfx950) GSO + DFIRE/DNA pose-energy engine.
 *
 * This is the drop-in boundary for ONE path of lightdock-rust v0.3.2: the scoring
 * functions behind `trait Score` and the GSO step that drives them.  Every entry point
 * names the reference interface it replaces (paths relative to the reference tree).
 * Plain pointers and sizes only; all floating point is IEEE f64 like the reference.
 *
 * Conventions
 *  - Functions returning `int` return LD_OK (0) or a negative ld_status; functions
 *    returning a handle return NULL on failure.  ld_last_error() gives the message
 *    (thread local).  Where the reference panics (exit 101) this library fails the call.
 *  - The caller keeps ownership of every input array (copied at create); outputs are
 *    written into caller-provided buffers.
 *  - A handle is bound to the HIP device current at create time and to one stream
 *    (ld_scorer_set_stream); it is thread-compatible, not thread-safe, like a
 *    `&Box<dyn Score>` used from the reference's single worker thread.
 *  - There is NO CPU fallback: without a usable HIP device create fails loudly.
 *
 * Pose row layout (== one line of initial_positions_N.dat, src/swarm.rs:36-52):
 *    [tx ty tz qw qx qy qz | rec_nm[anm_rec] | lig_nm[anm_lig]]     (f64, row-major)
 */
#ifndef LIGHTDOCK_HIP_H
#define LIGHTDOCK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum ld_status {
    LD_OK = 0,
    LD_ERR_INVALID = -1,     /* bad argument / inconsistent sizes */
    LD_ERR_UNSUPPORTED = -2, /* residue/atom/method the scoring function does not know */
    LD_ERR_IO = -3,          /* file missing / unreadable / malformed */
    LD_ERR_DEVICE = -4,      /* HIP error or no gfx950 device */
    LD_ERR_NOMEM = -5,
    LD_ERR_INTERNAL = -6     /* an iteration of the library's own did not end within its bound */
} ld_status;

/* src/scoring.rs:5-9 `enum Method` */
/* PYDOCK (src/pydock.rs) is the DNA energy (src/pydock.rs:425-545 == src/dna.rs:411-529) behind a
 * model builder with a generic-element fallback for unknown atoms (src/pydock.rs:332-345). */
typedef enum ld_method { LD_METHOD_DFIRE = 0, LD_METHOD_DNA = 1, LD_METHOD_PYDOCK = 2 } ld_method;

#define LD_DFIRE_TABLE_LEN (169 * 169 * 20) /* src/dfire.rs:216,251 */

const char *ld_last_error(void);
const char *ld_version(void);

/* Select the HIP device for handles created afterwards on this thread (hipSetDevice).
 * No counterpart in the reference (CPU only).  device < 0: $LIGHTDOCK_DEVICE or 0. */
int ld_init(int device);
int ld_device_count(void);

/* ------------------------------------------------------------------------------------
 * Scorer construction from arrays: what a Rust `impl Score` shim hands over after it has
 * run its own model builder.  Replaces DFIRE::new / DNA::new
 * (src/dfire.rs:201-234, src/dna.rs:375-408) minus the PDB walk.
 * ---------------------------------------------------------------------------------- */
typedef struct ld_molecule {
    size_t n_atoms;
    const double *coordinates;        /* n_atoms x 3, == DockingModel.coordinates (src/dfire.rs:106) */
    const uint32_t *dfire_types;      /* DFIRE: DockingModel.atoms, 0..167 (src/dfire.rs:105); else NULL */
    const double *ele_charges;        /* DNA: src/dna.rs:245; else NULL */
    const double *vdw_charges;        /* DNA: src/dna.rs:244 */
    const double *vdw_radii;          /* DNA: src/dna.rs:243 */
    size_t n_membrane;                /* DockingModel.membrane (src/dfire.rs:107): atom indices of MMB.BJ beads */
    const uint32_t *membrane;
    size_t n_restraint_groups;        /* DockingModel.active_restraints (src/dfire.rs:108) as CSR: */
    const uint32_t *restraint_offsets;/*   n_restraint_groups + 1 offsets into restraint_atoms */
    const uint32_t *restraint_atoms;  /*   atom indices, one group per restraint residue found in the PDB */
    size_t num_anm;                   /* DockingModel.num_anm */
    const double *nmodes;             /* num_anm x n_atoms x 3, C order (src/dfire.rs:292-299); NULL if num_anm == 0 */
} ld_molecule;

typedef struct ld_scorer_desc {
    int method;              /* ld_method */
    int use_anm;             /* DFIRE.use_anm / DNA.use_anm */
    ld_molecule receptor;
    ld_molecule ligand;
    const double *potential; /* DFIRE: LD_DFIRE_TABLE_LEN values of data/DCparams (src/dfire.rs:236-257) */
} ld_scorer_desc;

typedef struct ld_scorer ld_scorer;

ld_scorer *ld_scorer_create(const ld_scorer_desc *desc);

/* Same, but with the host-side model builder of this library doing the PDB walk, atom
 * typing and restraint lookup: DFIRE::new / DNA::new including DFIREDockingModel::new
 * (src/dfire.rs:115-190) and DNADockingModel::new (src/dna.rs:249-364).  Restraint ids are
 * "chain.resname.serial[icode]" strings (src/dfire.rs:139-142).  Passive lists are accepted
 * and ignored exactly like the reference (src/dfire.rs:164-175, never read by energy).
 * nmodes arrays are the flat contents of rec_nm.npy / lig_nm.npy (may be NULL, len 0). */
ld_scorer *ld_scorer_create_from_pdb(int method, const char *receptor_pdb, const char *ligand_pdb,
                                     const char *const *rec_active, size_t n_rec_active,
                                     const char *const *rec_passive, size_t n_rec_passive,
                                     const double *rec_nmodes, size_t rec_nmodes_len, size_t rec_num_anm,
                                     const char *const *lig_active, size_t n_lig_active,
                                     const char *const *lig_passive, size_t n_lig_passive,
                                     const double *lig_nmodes, size_t lig_nmodes_len, size_t lig_num_anm,
                                     int use_anm, const double *potential);

void ld_scorer_destroy(ld_scorer *s); /* Drop of the Box<dyn Score> */

/* ------------------------------------------------------------------------------------
 * Host-side model builder on its own (no GPU needed): DFIREDockingModel::new
 * (src/dfire.rs:115-190) / DNADockingModel::new (src/dna.rs:249-364).  The returned view
 * borrows the model's arrays and is what ld_scorer_create takes.
 * ---------------------------------------------------------------------------------- */
typedef struct ld_model ld_model;
ld_model *ld_model_from_pdb(int method, const char *pdb_path, const char *const *active, size_t n_active,
                            const char *const *passive, size_t n_passive, const double *nmodes, size_t nmodes_len,
                            size_t num_anm);
int ld_model_view(const ld_model *m, ld_molecule *out);
void ld_model_destroy(ld_model *m);
/* Residue labels in the model's atom order (host-side, no GPU): a residue is a maximal run of consecutive atoms of the
 * walk with one residue id, "<chain>.<resname>.<serial><icode>" (AtomRecord::residue_id, src/dfire.rs:139-142); indices
 * count runs in atom order, so ld_model_residue_of_atom is ascending and covers every atom.  It is the group map
 * ld_scorer_decompose takes for per-residue energies. */
size_t ld_model_num_residues(const ld_model *m);
int ld_model_residue_id(const ld_model *m, size_t index, char *buf, size_t buf_len);
int ld_model_residue_of_atom(const ld_model *m, uint32_t *out /* n_atoms */);

/* Host-side constants of the DFIRE kernel, exported for tests (DESIGN.md "bin LUT"):
 * the table bin DIST_TO_BINS[(sqrt(d2)*2-1) as usize]-1 (src/dfire.rs:49-53,336-337) of any
 * d2 in [0, 225] equals  b = lut[floor(4*d2)];  b += (d2 >= steps[b+1]);
 * lut: 901 cells of 0.25 A^2; steps[b], b = 0..20: first d2 the reference puts in bin >= b.
 * interface_d2: the largest d2 whose d = sqrt(d2)*2-1 is <= 3.9 (src/dfire.rs:339). */
int ld_dfire_bin_lut(uint8_t *lut_out /* 901 */, double *steps_out /* 21 */, double *interface_d2_out);
/* The cell LUT of the default DFIRE kernel, which tests pairs in f32 and recomputes in f64 only
 * where the f32 distance cannot decide the reference's result (host-side, no GPU; for tests).
 * With D' = cells_per_unit * 4 d2 + 1/2 evaluated in f32 on coordinates within `ubound` of the
 * frame centre (record units), word = words_out[min((unsigned)D', 1024 * cells_per_unit)]:
 *   word < 0x00800000            byte offset of the bin within a table patch: every f64 d2 that can
 *                                produce this cell has that bin, is inside the cutoff, sets no flag
 *   word == 0x00800000           every such d2 is beyond the cutoff (src/dfire.rs:334)
 *   word & 0x40000000            flagged: (word >> 24) & 15 == 1: one bin step exactly at the cell's
 *                                middle, bits 0..11 the offset below it, bits 12..23 its growth above;
 *                                other codes: decided by comparisons on the f64 distance.
 * eps_out: the bound on |D_f32 - 4 d2| (units of 4 d2) the LUT was built for.
 * words_out: 1028 * cells_per_unit entries; cells_per_unit is 1 or 2. */
int ld_dfire_packed_lut(int cells_per_unit, double ubound, uint32_t *words_out, double *eps_out);
/* The cell LUT of the block-major DFIRE kernels (kernels/dfire_bm.hpp; host-side, no GPU), for tests.  The kernel
 * computes E = 14583.5 - 64 d2 in f32 (error below eps_cells / 2, which depends on the frame `ubound` in record units
 * of 1/8 A and on the ligand's largest |local coordinate| `lig_extent` in A) and reads codes_out[floor(E)], E < 0 reading
 * cell 0:
 *   code 160                     every f64 d2 that can produce this cell is beyond the cutoff (src/dfire.rs:334)
 *   code 8 * bin, bin 0..19      every such d2 has that bin (src/dfire.rs:336-337) and is inside the cutoff: the byte offset of
 *                                the bin's slot in a table row of the kernel
 *   code 168                     flagged (the slot of the row's marker): the pair is recomputed in f64 -- a bin step or the
 *                                cutoff inside the cell's interval (hence r = 15.0 exactly, the reference's read past the row, :338)
 * codes_out: 14592 entries. */
int ld_dfire_bm_lut(double ubound, double lig_extent, uint8_t *codes_out, double *eps_cells_out);
/* The record frames the two culled DFIRE routes derive of a complex's coordinates (host-side, no GPU), for tests: the scorer's
 * own route predicates up to the frame, so a test that needs a frame of a given size asks instead of restating the rule.
 * anm: the complex flexes (the block-major ANM form keeps room for its deformations).  Either output may be NULL.
 * rec_types: the receptor's DFIRE types, with which its 8-atom subtiles are laid out as the scorer lays them out
 * (ld_dfire_tile_layout) and the widest subtile box enters the block-major bound; NULL: no subtile is taken to be wider than the
 * bound assumes (eps is then ld_dfire_bm_lut's for that frame).
 *   bm_out[9]      centre x y z (A), ubound (record units of 1/8 A), lig_extent (A), eps (LUT cells), 1.0 if eps < 8 (the
 *                  block-major route declines the complex otherwise) else 0.0, the widest receptor subtile box's half extent
 *                  along an axis and its half diagonal (record units, rounded up a little; 0 without rec_types)
 *   packed_out[8]  centre x y z, kappa (record units per A), ubound (record units), eps (units of 4 d2), LUT cells per unit of
 *                  4 d2, 1.0 if the pose-major packed route takes the receptor (the all-pairs kernel otherwise), else 0.0
 * LIGHTDOCK_PACKED_CELLS and LIGHTDOCK_PACKED_EPS_SCALE are read as the scorer reads them. */
int ld_dfire_route_frames(const double *rec_xyz /* n_rec x 3 */, const uint32_t *rec_types /* n_rec, or NULL */, size_t n_rec,
                          const double *lig_xyz /* n_lig x 3 */, size_t n_lig, int anm, double *bm_out /* 9 */, double *packed_out /* 8 */);
/* The fixed-point scale of that kernel (host-side, no GPU): table values enter a pose's sum as rint(v * scale), scale =
 * 2^(44 - e - x), 2^e >= table_vmax, integer adds in any order (the sum src/dfire.rs:325-345 takes in f64).  x makes the sum of
 * one (pose, ligand tile) -- 64 ligand atoms x the receptor atoms within `reach` = cutoff + the tile's radius of its centre --
 * fit 63 bits: reach_count_out = an upper bound on the receptor atoms inside ANY ball of that radius (n_rec itself below 8192
 * atoms: no search), x = extra_bits_out = the bits that count takes beyond 2^13.  scale_out = 0.0: no scale fits (a table
 * value beyond 1024 or not finite, or a count beyond 2^23) -- such a scorer runs the pose-major kernels. */
int ld_dfire_bm_fix_scale(const double *rec_xyz /* n_rec x 3 */, size_t n_rec, double reach, double table_vmax,
                          uint64_t *reach_count_out, int *extra_bits_out, double *scale_out);
/* The workspace of the block-major DFIRE kernels for one batch shape (host-side, no GPU), for tests: the layout the scorer
 * itself reserves and points its launches into (kernels/dfire_bm.hpp, bm_layout).  n_rt / n_lt: receptor / ligand tiles; cap:
 * poses per pass; sets: passes in flight (1 or 2); waves: waves of dfire_bm_pairs; flags: 1 = ANM form, 2 = counting launch,
 * 4 = LIGHTDOCK_BM_DEBUG.  For each of the 22 regions r: names_out[2 r] = its name, names_out[2 r + 1] = its
 * buffer's name (static strings), rows_out[5 r ..] = {buffer index, the buffer's bytes (slack included), byte offset of set 0,
 * byte stride from set to set, bytes of one set}.  A region the shape does not ask for has 0 bytes. */
int ld_dfire_bm_workspace(size_t n_rt, size_t n_lt, size_t cap, size_t sets, size_t waves, int flags,
                          const char **names_out /* 2 x 22 */, uint64_t *rows_out /* 5 x 22 */);
/* The atom order the culled DFIRE kernels use (host-side, no GPU): order_out[slot] = original atom
 * index, UINT32_MAX for padding; length = ceil(n/64)*64.  Consecutive 8 slots ("subtile") and 64
 * slots ("tile") are spatially compact; padding only at the tail.  The energy is a plain sum over
 * pairs (src/dfire.rs:325-345), so the order is free.  Returns the padded length. */
size_t ld_spatial_tile_order(const double *xyz /* n x 3 */, size_t n, uint32_t *order_out);
/* The complete layout the DFIRE scorer uses for one molecule (host-side, no GPU): the order above
 * refined so that atom types which share a 128-byte patch of the re-laid-out potential sit in the
 * same subtile, and the renumbering of the DFIRE types (type_perm_out[type] = number in the patch
 * layout; 2k and 2k+1 share patches).  order_out: ceil(n/64)*64 entries, type_perm_out: 169.
 * Returns the padded length. */
size_t ld_dfire_tile_layout(const double *xyz /* n x 3 */, const uint32_t *dfire_types /* n */, size_t n,
                            uint32_t *order_out, uint32_t *type_perm_out);

/* rand 0.7.3 StdRng::seed_from_u64 -> the 8 ChaCha20 key words the GSO kernel uses (src/lib.rs:38). */
void ld_stdrng_key(uint64_t seed, uint32_t key_out[8]);

/* DFIRE::load_potentials (src/dfire.rs:236-257): first 169*169*20 lines of a text file. */
int ld_load_dcparams(const char *path, double *out /* LD_DFIRE_TABLE_LEN */);

/* introspection (host copies of what the model builder produced) */
size_t ld_scorer_num_atoms(const ld_scorer *s, int side /* 0 receptor, 1 ligand */);
size_t ld_scorer_pose_len(const ld_scorer *s);  /* 7, or 7 + anm_rec + anm_lig when use_anm */
int ld_scorer_method(const ld_scorer *s);
int ld_scorer_model_arrays(const ld_scorer *s, int side, double *coordinates /* n*3 or NULL */,
                           uint32_t *dfire_types /* n or NULL */, double *ele_charges, double *vdw_charges,
                           double *vdw_radii);

/* Bind the handle to a HIP stream (hipStream_t passed as void*); NULL = the default
 * stream.  All *_device calls and kernels of this handle are enqueued there. */
int ld_scorer_set_stream(ld_scorer *s, void *hip_stream);

/* `Score::energy` (src/scoring.rs:11-19; impls src/dfire.rs:264-363, src/dna.rs:410-529):
 * one pose in, one f64 out; rec_nm / lig_nm may be NULL when the scorer has no ANM.
 * Synchronous (host pointers). */
int ld_scorer_energy(ld_scorer *s, const double translation[3], const double rotation_wxyz[4],
                     const double *rec_nmodes, const double *lig_nmodes, double *energy_out);

/* Batched form of the same call: what Swarm::update_luciferin (src/swarm.rs:66-70) does
 * one glowworm at a time.  poses: n rows of `stride` doubles (stride >= pose_len).
 * Host-pointer version copies in/out and synchronises.
 *
 * The results of every ld_scorer entry -- energies, pair counts, decompositions, refinements -- do not depend on earlier
 * calls on the handle, whatever their size, options or outcome: the handle's device workspace only grows and is shared by
 * all of them, but a call reads nothing that it has not written itself, and a refused call (LD_ERR_INVALID) writes no
 * output and leaves the handle as it was.  A pose's energy is the same bits in every batch, on a new handle and on a used one. */
int ld_scorer_energy_batch(ld_scorer *s, size_t n, const double *poses, size_t stride, double *energies_out);

/* Device-pointer version: poses and energies already live in HBM (hipMalloc / a torch CUDA
 * tensor's data_ptr); asynchronous on the handle's stream.  `active` (device, n bytes, may
 * be NULL) skips poses whose byte is 0 and leaves their output untouched -- this is the
 * `if self.moved || self.step == 0` of Glowworm::compute_luciferin (src/glowworm.rs:62).
 * `pair_counts` (device, n x uint32, may be NULL) receives the number of atom pairs inside
 * the outer cutoff (DFIRE d2 <= 225, src/dfire.rs:334; DNA d2 <= 900, src/dna.rs:481): the
 * P_cut of the algorithmic-bytes model. */
int ld_scorer_energy_batch_device(ld_scorer *s, size_t n, const double *d_poses, size_t stride,
                                  const uint8_t *d_active, double *d_energies_out, uint32_t *d_pair_counts);

/* Diagnostics of the box-culled DFIRE kernels (block-major and pose-major): after a
 * ld_scorer_energy_batch_device call WITH pair_counts, the number of 8x8 atom-pair blocks each of
 * those n poses actually evaluated (64 pair tests each; compare with n_rec*n_lig/64 for all pairs).
 * Synchronises.  Returns LD_ERR_UNSUPPORTED for scorers that run the all-pairs kernel (DNA,
 * LIGHTDOCK_DFIRE_KERNEL=allpairs, receptors too long for the packed f32 frame). */
int ld_scorer_last_block_counts(ld_scorer *s, size_t n, uint32_t *blocks_out_host);

/* Diagnostics of the block-major DFIRE path: the number of receptor subtiles (8 atoms of the tile order) whose atoms' rows of the
 * potential -- atoma * 169 * 20 + atomb * 20 + bin, src/dfire.rs:338, all 20 bins and the read past the row at r = 15.0 -- are 0.0
 * against every ligand type of the complex (membrane beads, if the DCparams at hand has zero rows for them).  Such a subtile adds
 * nothing to any sum: the culling lists its blocks within the interface distance only (r <= 2.45 A, src/dfire.rs:339; never, when
 * neither it nor the ligand holds a restraint atom or a bead).  0 for a table without such rows and for the other kernels. */
int ld_scorer_bm_quiet_subtiles(const ld_scorer *s, uint32_t *count_out);

/* Diagnostics of the block-major DFIRE path: how a batch of n poses would run on this handle.  pass_poses_out: the poses of a pass,
 * min(n, the pass size the scorer derived when it was built); sets_out: the workspace sets, 2 when the batch takes several passes
 * (they alternate between two streams), else 1.  A batch of one pass that wants no pair counts runs the fused launch sequence.
 * Either output may be NULL; both are 0 for a scorer of another route.  Launches nothing. */
int ld_scorer_bm_passes(const ld_scorer *s, size_t n, size_t *pass_poses_out, size_t *sets_out);

/* Per-launch facts for the measurement harness. */
typedef struct ld_kernel_info {
    const char *pair_kernel_name; /* symbol of the dominant (pair loop) kernel */
    uint32_t block_threads;
    uint32_t receptor_chunks;     /* workgroups per pose */
    uint32_t lds_bytes;
    uint64_t pair_tests_per_pose; /* n_rec * n_lig */
    uint64_t stream_bytes_per_pose; /* algorithmic bytes excluding the 8*P_cut gather term */
} ld_kernel_info;
int ld_scorer_kernel_info(const ld_scorer *s, ld_kernel_info *out);

/* Measurement hook: when enabled, every ld_scorer_energy_batch_device call brackets its
 * pair kernel with HIP events on the handle's stream.  ld_scorer_pair_kernel_time
 * synchronises those events and returns the summed duration (ms) and launch count since
 * the last reset; reading also resets. */
int ld_scorer_enable_timing(ld_scorer *s, int enable);
int ld_scorer_pair_kernel_time(ld_scorer *s, double *total_ms_out, uint64_t *launches_out);

/* ------------------------------------------------------------------------------------
 * Energy decomposition: which terms make up a pose's energy, and which atoms or groups of atoms (residues) carry it.
 * Its own kernels with a defined order of every sum, so a pose's results are the same bits whatever the batch, its place
 * in it, the launch shape or the pass size.  The definition:
 *   Posing: as the energy path, ligand atom q v q^-1 + t, then both molecules' ANM terms in ascending mode order
 *     (src/dfire.rs:282-320, src/qt.rs:57-61); d2 = dx dx + dy dy + dz dz, left to right, unfused, dx = receptor - ligand.
 *   Pair of receptor atom i and ligand atom j, DFIRE (src/dfire.rs:334-343): if d2 <= 225 the pair counts and contributes
 *     v = potential[type_i * 3380 + type_j * 20 + bin], bin = DIST_TO_BINS[(sqrt(d2) * 2 - 1) as usize] - 1, which at
 *     r = 15.0 reads past the row like the reference; the pair is interface iff sqrt(d2) * 2 - 1 <= 3.9.
 *   DNA / PYDOCK (src/dna.rs:476-511), true f64 divisions, the reference's comparisons (a NaN stays a NaN):
 *     d2 <= 900: e = q_i q_j / d2, e > 4/332 -> 4/332, e < -4/332 -> -4/332; the pair counts and contributes e to term 0;
 *     d2 <= 100: p6 = powi(r_i + r_j, 6) / powi(d2, 3), k = sqrt(eps_i eps_j) (p6 p6 - 2 p6), k > 1 -> 1; k to term 1;
 *     d2 <= 3.9 * 3.9: interface.   powi(x, 6) = x2 (x2 x2), x2 = x x;  powi(x, 3) = x x x.
 *   Atom of either side: per term (DFIRE 1, DNA / PYDOCK 2) the f64 sum of its pairs' contributions taken sequentially in
 *     ascending partner index from 0.0; the number of its counting pairs; whether any of its pairs is interface.
 *   Group: the sequential sum from 0.0, in ascending atom index, of its atoms' sums, counts and flags.
 *   Pose (ld_energy_terms): pair[k] = the RECEPTOR atoms' sums of term k added in ascending atom order from 0.0;
 *     score = (pair[0] * 0.0157 - 4.7) * -1 (src/dfire.rs:347) or (pair[0] * 332 / 4 + pair[1]) * -1 (src/dna.rs:513-514);
 *     rec_restraints, lig_restraints, membrane: the fractions of src/scoring.rs:21-47 over the per-atom flags (0 without
 *     restraints / beads); energy = score + rec_restraints * score + lig_restraints * score - penalty, penalty =
 *     999 * membrane where membrane > 0 (src/dfire.rs:349-361); pairs, rec_interface, lig_interface: counting pairs and
 *     flagged atoms.
 * Every pair is evaluated twice, once for each of its atoms.  Poses run in passes of at most `slice` poses
 * (ld_scorer_decompose_info), slice = clamp(64 MiB / per-pose workspace bytes, 1, 4096); a lane owns one atom and walks the
 * other molecule through LDS in chunks, whose size changes no sum.
 * ---------------------------------------------------------------------------------- */
#define LD_GROUP_NONE (0xffffffffu) /* atom belongs to no group */
typedef struct ld_energy_terms {
    double pair[2];        /* DFIRE: [1] is 0 */
    double score;
    double rec_restraints;
    double lig_restraints;
    double membrane;
    double energy;
    uint32_t pairs;
    uint32_t rec_interface;
    uint32_t lig_interface;
    uint32_t reserved;     /* 0 */
} ld_energy_terms;
typedef struct ld_group_energies { /* one side; any pointer may be NULL */
    const uint32_t *group_of_atom; /* n_atoms(side), values < n_groups or LD_GROUP_NONE; NULL: every atom its own group, n_groups is then taken as n_atoms(side) */
    size_t n_groups;
    double *sums;                  /* n x n_groups x 2 (DFIRE: [1] is 0) */
    uint32_t *pairs;               /* n x n_groups */
    uint32_t *interface_atoms;     /* n x n_groups */
} ld_group_energies;
/* Host pointers, synchronous.  poses: n rows of `stride` >= pose_len doubles.  n == 0 is LD_OK and touches nothing.  Groups
 * need not be contiguous; an empty group yields zeros.  LD_ERR_INVALID, every output as it was: stride < pose_len, a group
 * id >= n_groups, n_groups == 0 with a map (both also where none of that side's rows is asked for), n x n_groups x 16
 * beyond a size_t, poses missing.  Device staging beyond the workspace: slice x n_groups x 24 B a side. */
int ld_scorer_decompose(ld_scorer *s, size_t n, const double *poses, size_t stride,
                        ld_energy_terms *terms_out /* n, may be NULL */,
                        const ld_group_energies *receptor /* may be NULL */,
                        const ld_group_energies *ligand /* may be NULL */);
/* Either output may be NULL.  last_kernel_ms: the kernels of the last ld_scorer_decompose call, all passes (HIP events). */
int ld_scorer_decompose_info(const ld_scorer *s, size_t *slice_poses_out, double *last_kernel_ms_out);

/* ------------------------------------------------------------------------------------
 * Local refinement: walk a pose uphill under the scorer's own energy by a compass search, every decision a rule without
 * randomness or line search, so a host restatement follows it to the bit.  The definition:
 *   A pose is [t(3) | q wxyz(4) | extents(pose_len - 7)] as the scorer reads it; energies are the scorer's own
 *     (ld_scorer_energy_batch_device); higher is better, as in the GSO.  Per pose the state is E, dt, c, s, dn, halvings, frozen.
 *   Start: E = the pose's energy; dt = trans_step, dn = nm_step; c = cos(rot_step / 2), s = sin(rot_step / 2), taken once on
 *     the host with std::cos / std::sin; halvings = 0.
 *   Trials of one iteration, K = 12 + 2 (pose_len - 7), in this order:
 *     j = 2 k + sigma, k = 0..2: t[k] + dt for sigma = 0, t[k] - dt for sigma = 1;
 *     j = 6 + 2 k + sigma: q' = r q with r = (c, +-s on axis k, 0 elsewhere), +s for sigma = 0; the product is Quaternion::mul
 *       (src/qt.rs:177-184), the same expression in the same order, unfused, and q' is not normalised.  A left product turns
 *       the ligand about the origin of its own coordinates, because the energy path poses it as q v q^-1 + t;
 *     j = 12 + 2 m + sigma: extent[m] +- dn.
 *     Everything else in a trial row is the pose's bits.
 *   Choice: NaN trial energies count as -inf; j* is the first index of the maximum; accept iff e[j*] > E, strictly.  On accept
 *     the pose becomes trial j*, E = e[j*], and the steps stay.
 *   Failure with halvings < max_halvings: halvings += 1; dt *= 0.5, dn *= 0.5; c' = sqrt((1 + c) 0.5), s = s / (2 c'),
 *     c = c' (IEEE add, multiply, divide and sqrt only).
 *   Failure with halvings == max_halvings: the pose is frozen, and never evaluated or touched again.
 *   History, one ld_refine_history per pose and iteration: j* on an accept, -1 when halved, -2 when frozen in this
 *     iteration, -3 when not evaluated.   evaluations = 1 + K x (iterations in which the pose was evaluated).
 * A pose whose start energy is NaN (non-finite input, zero quaternion) therefore comes back with its own bits.
 * Poses run in passes of `slice` poses (slice x K <= 65 536 trial rows unless slice_poses names it; at most 2^22 rows), each
 * pass all its iterations: one start-energy launch, then refine_trials, the energy launch over the pass's trial rows by their
 * mask, refine_select per iteration, on the scorer's stream without a host synchronisation in between.
 * ---------------------------------------------------------------------------------- */
typedef int16_t ld_refine_history;
typedef struct ld_refine_options {
    uint32_t iterations;
    uint32_t max_halvings;
    double trans_step;    /* A */
    double rot_step;      /* rad, <= pi */
    double nm_step;       /* extent units */
    uint32_t slice_poses; /* 0: the library's */
    uint32_t reserved;    /* 0 */
} ld_refine_options;
typedef struct ld_refine_stats {
    double energy_before;
    double energy_after;
    uint32_t accepted;
    uint32_t halvings;
    uint32_t evaluations;
    uint32_t frozen;
} ld_refine_stats;
typedef struct ld_refine_state { /* per pose: host arrays of n */
    double *energy;
    double *trans_step;
    double *rot_cos;
    double *rot_sin;
    double *nm_step;
    uint32_t *halvings;
    uint32_t *accepted;
    uint32_t *evaluations;
    uint8_t *frozen;
} ld_refine_state;
/* Host pointers, synchronous.  poses: n rows of `stride` >= pose_len doubles.  n == 0 is LD_OK and touches nothing.
 * LD_ERR_INVALID, every output as it was: iterations == 0, a step that is not finite and > 0, rot_step > pi,
 * stride < pose_len, poses or poses_out missing with n > 0, slice_poses x K beyond 2^22, any size beyond a size_t. */
int ld_scorer_refine(ld_scorer *s, const ld_refine_options *opts, size_t n, const double *poses, size_t stride,
                     double *poses_out /* n x pose_len */, ld_refine_stats *stats_out /* n, or NULL */,
                     ld_refine_history *history_out /* n x iterations, or NULL */);
/* Any output may be NULL.  trials: K of this scorer; slice: the poses per pass of the last call (before any: the default);
 * last_kernel_ms: the device work of the last call, all passes (HIP events); evaluations: its total over all poses. */
int ld_scorer_refine_info(const ld_scorer *s, size_t *trials_out, size_t *slice_poses_out, double *last_kernel_ms_out,
                          uint64_t *evaluations_out);
/* Host only: K, the poses per pass and the device workspace of a call (any output may be NULL).  LD_ERR_INVALID: pose_len
 * outside 7 .. 135, stride < pose_len, iterations == 0, slice_poses x K beyond 2^22, a size beyond a size_t. */
int ld_refine_plan(size_t pose_len, size_t n, size_t stride, uint32_t iterations, uint32_t slice_poses, size_t *trials_out,
                   size_t *slice_poses_out, size_t *workspace_bytes_out);
/* The two kernels of an iteration on caller-given state, without a scorer (host pointers, synchronous; what the tests hold
 * to the restatement).  ld_refine_trials: trial j of pose p goes to trials + (p K + j) trial_stride, its first pose_len
 * doubles; active: n x K bytes, 1 for an unfrozen pose and 0 for a frozen one, whose rows stay as they were.
 * ld_refine_select: energies n x K (a frozen pose's row is not read); poses and state are updated in place;
 * history_out: n entries. */
int ld_refine_trials(size_t n, size_t pose_len, const double *poses, size_t stride, const ld_refine_state *state,
                     double *trials /* n x K x trial_stride, in and out */, size_t trial_stride, uint8_t *active_out);
int ld_refine_select(size_t n, size_t pose_len, double *poses, size_t stride, const ld_refine_state *state,
                     const double *energies, uint32_t max_halvings, ld_refine_history *history_out);

/* ------------------------------------------------------------------------------------
 * GSO: batched over independent swarms.  Replaces GSO::new / GSO::run
 * (src/lib.rs:27-58), Swarm (src/swarm.rs) and Glowworm (src/glowworm.rs).
 * ---------------------------------------------------------------------------------- */
typedef struct ld_gso ld_gso;

/* positions: n_swarms x n_glowworms rows of pose_len doubles (src/swarm.rs:26-64).
 * seeds: one u64 per swarm (GSO::new's `seed`, src/lib.rs:38), or NULL for DEFAULT_SEED
 * 324324 (src/constants.rs:2) everywhere.
 * Several ld_gso may share one ld_scorer, and other calls on that scorer may come between their steps: they use its
 * workspace one after the other (calls on one scorer are not thread-safe), and a GSO's state does not depend on them. */
ld_gso *ld_gso_create(ld_scorer *scorer, size_t n_swarms, size_t n_glowworms, const double *positions,
                      const uint64_t *seeds);
void ld_gso_destroy(ld_gso *g);

/* One iteration of the loop body of GSO::run (src/lib.rs:47-50): update_luciferin
 * (pose-energy kernel over the glowworms that moved) then movement_phase.  Asynchronous. */
int ld_gso_step(ld_gso *g);
/* `steps` iterations back to back (hipGraph replay when available). */
int ld_gso_run(ld_gso *g, uint32_t steps);
uint32_t ld_gso_steps_done(const ld_gso *g);
uint64_t ld_gso_num_evals(ld_gso *g); /* energy evaluations so far, all swarms (synchronises) */

/* Snapshot of one swarm (synchronises).  Any pointer may be NULL.
 * poses: n_glowworms x pose_len; neighbors = neighbour count of the last movement phase. */
int ld_gso_read(ld_gso *g, size_t swarm, double *poses, double *luciferin, double *vision_range,
                double *scoring, int32_t *n_neighbors, int32_t *moved, int32_t *target);

/* Swarm::save (src/swarm.rs:128-167): writes "<dir>/gso_<step>.out" for one swarm. */
int ld_gso_save(ld_gso *g, size_t swarm, uint32_t step, const char *dir);
/* The same for many swarms of one ld_gso at once (what a multi-swarm launcher does after a save
 * step): dirs[k] receives swarm swarms[k].  The state is copied from the device once and the files
 * are written by a few host threads. */
int ld_gso_save_many(ld_gso *g, size_t n, const size_t *swarms, const char *const *dirs, uint32_t step);

/* ------------------------------------------------------------------------------------
 * Analysis of a finished run (example/1czy/analysis.sh: lgd_cluster_bsas.py, lgd_top.py);
 * no scoring model needed.  Atoms: the ATOM/HETATM records of the two PDB files in FILE order
 * (other records are dropped).  Modes: lightdock_<side>.nm.npy flattened, num_anm x atoms x 3.
 * Posing at [t | q | rec_ext | lig_ext] (NOT the energy's convention, src/dfire.rs:283-300):
 *   receptor atom a:  R_a + sum_m rec_ext[m] * rec_mode[m][a]
 *   ligand atom a:    rotate(q, L_a + sum_m lig_ext[m] * lig_mode[m][a]) + t   (src/qt.rs:48-61)
 * LD_ERR_INVALID, nothing written: non-finite poses or scores, a zero quaternion, modes whose
 * length is not num_anm x atoms x 3, no atom named CA or P (clustering), n_glowworms 0 or > 4096.
 * What a call on a handle returns does not depend on what the handle ran or refused before, whichever of the calls
 * below (tests/test_gpu_handle_history.py; tests/asan/history_check.cpp for the host side).
 * ---------------------------------------------------------------------------------- */
typedef struct ld_complex ld_complex;

ld_complex *ld_complex_create(const char *receptor_pdb, const char *ligand_pdb,
                              const double *rec_nmodes, size_t rec_nmodes_len, size_t rec_num_anm,
                              const double *lig_nmodes, size_t lig_nmodes_len, size_t lig_num_anm);
void ld_complex_destroy(ld_complex *c);
size_t ld_complex_pose_len(const ld_complex *c); /* 7 + rec_num_anm + lig_num_anm */
size_t ld_complex_num_atoms(const ld_complex *c, int side); /* 0 receptor, 1 ligand, 2 CA / P atoms of the complex */
/* poses: n rows of `stride` >= pose_len doubles; xyz_out: n x (n_rec + n_lig) x 3, unrounded */
int ld_complex_coordinates(ld_complex *c, size_t n, const double *poses, size_t stride, double *xyz_out);
/* lgd_cluster_bsas.py for every swarm at once: per swarm, glowworms sorted by scoring (highest
 * first, ties in glowworm order) each join the FIRST cluster whose founder is within
 * round(rmsd, 4) <= cutoff, else found one; rmsd over the complex's CA / P atoms, no superposition,
 * coordinates rounded as "%8.3f" prints them.  representatives: founders in creation order, -1
 * after the last.  Device workspace: at most 256 MiB, or one swarm's n_glowworms x n_CA/P x 12 B. */
int ld_complex_cluster(ld_complex *c, size_t n_swarms, size_t n_glowworms, const double *poses, size_t stride,
                       const double *scoring, double cutoff,
                       int32_t *cluster_of /* n_swarms x n_glowworms */,
                       int32_t *representatives /* n_swarms x n_glowworms */,
                       uint32_t *n_clusters /* n_swarms */);
int ld_complex_last_kernel_ms(const ld_complex *c, double *ms_out); /* kernels of the last cluster, contacts or assess call (HIP events) */
/* lgd_top.py: receptor then ligand ATOM/HETATM lines as line[:30] + "%8.3f%8.3f%8.3f" + line[54:] */
int ld_complex_write_pdb(ld_complex *c, const double *pose, const char *path);

/* Clustering a ranked list: ld_complex_cluster's rule for ONE list of poses of any swarms, up to about a million,
 * in several workgroups; what removes the models that neighbouring swarms found independently.
 *   Order: the poses are taken by (scoring descending, index ascending).
 *   Rule: a pose joins the FIRST representative, in creation order, for which within_cutoff holds; if none does it
 *     becomes the next representative.
 *   within_cutoff: rint(sqrt(S * 1e-6 / n_atoms) * 1e4) / 1e4 <= cutoff, S the sum of the squared differences of the
 *     thousandths "%.3f" prints of the posed atoms (posing and rounding as above): ld_complex_cluster's predicate.
 *   atoms = 0: the CA / P atoms of the whole complex, BSAS's measure; for n <= 4096 the three outputs equal
 *     ld_complex_cluster(c, 1, n, ...)'s word for word.  atoms = 1: the ligand's CA / P atoms only, n_atoms their
 *     count, so that the receptor does not dilute the measure.
 *   Outputs: cluster_of in input order; representatives: input indices in creation order, -1 after the last;
 *     n_clusters: one word.  n == 0 is LD_OK and sets *n_clusters = 0.
 *   Equality with the sequential rule is owed wherever S < 2^53: below it the sum is exact, hence order-free.
 * LD_ERR_INVALID, nothing written: a NaN cutoff, atoms other than 0 / 1, a non-finite scoring or pose value, a zero
 * quaternion, no CA / P atom in the chosen set, a posed coordinate beyond an int32 of thousandths (+-2.1e6 A), a list
 * whose device workspace, n x walked atoms x 12 B, would exceed 4 GiB (walked atoms: the chosen set, less the
 * receptor's when atoms = 0 and the receptor has no modes: they cannot move).  The bound is checked before the list
 * is read.  ld_complex_last_kernel_ms then reports this call from its first launch to its last, host rounds included. */
int ld_complex_cluster_ranked(ld_complex *c, size_t n, const double *poses, size_t stride, const double *scoring,
                              double cutoff, int atoms, int32_t *cluster_of /* n */, int32_t *representatives /* n */,
                              uint32_t *n_clusters /* 1 */);

/* Interface contacts: for every pose, which receptor and which ligand residues touch.  The primitive
 * under LightDock's lgd_filter_restraints.py and lgd_filter_membrane.py, which re-read the PDB file of
 * a model and compare a distance matrix with a cutoff; those tools are not part of the reference
 * tree, so the rule below is this library's own definition, modelled on them.
 *   Residues: a residue is a maximal run of consecutive ATOM/HETATM records (file order) with the same
 *     residue name (columns 18-20), chain (22), sequence number (23-26) and insertion code (27).  Its
 *     id is AtomRecord::residue_id() (src/dfire.rs:139-142), "<chain>.<resname>.<serial><icode>",
 *     e.g. A.SER.467, H.ASP.52A.  Indices count runs in file order, receptor and ligand separately.
 *   Posing: as above (f64, reference operation order); every coordinate is then the integer number
 *     of thousandths that "%8.3f" prints, so the contacts of a pose are those of the file
 *     ld_complex_write_pdb writes for it.
 *   Contact: C = llrint(cutoff * 1000), 1 <= C <= 30000.  Receptor atom a and ligand atom b touch iff
 *     dx^2 + dy^2 + dz^2 <= C^2 in exact integer arithmetic on the thousandths.  A residue is in
 *     contact iff any of its atoms touches any atom of the other molecule.  All atoms count
 *     (hydrogens, hetero atoms, membrane beads).  No floating-point comparison decides anything.
 * Bit k of word w of a pose's row is residue 32 w + k; bits beyond the last residue are 0.
 * LD_ERR_INVALID, nothing written: non-finite poses, a zero quaternion, stride < pose_len, a cutoff
 * that is NaN or whose C is outside 1 .. 30000, a side other than 0 / 1, a buffer too short for an
 * id, a posed coordinate beyond +-1.0e6 A (so that the difference of two coordinates fits an int32).
 * Replaces the distance-matrix pass of lgd_filter_restraints.py / lgd_filter_membrane.py over per-model
 * PDB files.  Device workspace: one slot of atoms x 16 B (plus 24 B a residue and a group of 8 ligand
 * residues when those boxes exceed 40 KiB) per workgroup in flight, at most 1024 slots and 256 MiB (or one slot). */
size_t ld_complex_num_residues(const ld_complex *c, int side); /* 0 receptor, 1 ligand */
int ld_complex_residue_id(const ld_complex *c, int side, size_t index, char *buf, size_t buf_len);
int ld_complex_residue_of_atom(const ld_complex *c, int side, uint32_t *out /* n_atoms of that side */);
/* Either output may be NULL; n == 0 is LD_OK.  ld_complex_last_kernel_ms then reports this call's kernels. */
int ld_complex_contacts(ld_complex *c, size_t n, const double *poses, size_t stride, double cutoff,
                        uint32_t *rec_bits /* n x ceil(n_rec_res / 32) */,
                        uint32_t *lig_bits /* n x ceil(n_lig_res / 32) */);

/* Clustering by common contacts: models grouped by what their interface is made of -- the fraction of common contacts
 * (FCC) of HADDOCK's cluster_fcc.py -- and a CONSRANK-style consensus score, how often a model's residue pairs recur over
 * all the models.  This library's own rule, modelled on those two; no byte compatibility with an outside tool is claimed.
 * Everything is integer arithmetic, so a result is the same bits whatever the batch or the schedule.
 *   Pair set of a pose: residues, posing, rounding and the atom test are exactly those of "Interface contacts" (posed f64,
 *     integer thousandths, C = llrint(cutoff * 1000), 1 <= C <= 30000, d^2 <= C^2 in exact integers, all atoms count).
 *     P_i is the set of keys r * n_lig_res + l, r a receptor and l a ligand residue index; a key is in the set when some
 *     atom of r touches some atom of l.  Keys are uint32_t: a complex with n_rec_res * n_lig_res >= 2^32 is refused.  A
 *     pose's keys are emitted in ascending order.  The projection of P_i onto either side is, word for word, that pose's
 *     row of ld_complex_contacts at the same cutoff.
 *   Common contacts: s_i = |P_i|, c_ij = |P_i & P_j|.
 *   Neighbours: T = llrint(threshold * 1000), 1 <= T <= 1000.  For i != j, poses i and j are neighbours iff s_i > 0,
 *     s_j > 0 and 1000 * c_ij >= T * max(s_i, s_j) in 64-bit integers: FCC with strictness 1, a symmetric relation.  A
 *     pose with an empty set has no neighbours.
 *   Clusters: all poses start alive.  Until no pose is alive: (1) for every alive pose d_i = 1 + the number of its alive
 *     neighbours; (2) the centre is the alive pose with the largest d, ties to the larger scoring, then to the smaller
 *     index; (3) if that d < min_size (min_size >= 1) the repetition stops and every pose still alive gets cluster -1;
 *     (4) otherwise the centre and its alive neighbours form the next cluster and die.  Clusters are numbered in creation
 *     order, so their sizes never increase.
 *   Outputs, as ld_complex_cluster_ranked's: cluster_of (n, -1 for unclustered), centres (n, input indices in creation
 *     order, -1 after the last), n_clusters (one word).
 *   Consensus: freq[k] is the number of poses whose set holds key k; consensus_i is the sum of freq[k] over k in P_i.  The
 *     fraction is consensus_i / (s_i * n), and 0 for an empty set: the caller's arithmetic.
 * LD_ERR_INVALID, nothing written: everything ld_complex_contacts refuses; a non-finite scoring; a threshold that is NaN or
 * whose T is outside 1 .. 1000; min_size == 0; for the entries that take sets from the caller, offsets that do not start
 * at 0 or do not ascend and keys that are not strictly ascending within a set; a cap below the number of keys; a list
 * beyond the workspace bounds: more than 65536 sets to cluster (the neighbour bits, n^2 / 8 B, stay within 512 MiB), more
 * than 16384 sets for ld_fcc_common (n x n words within 1 GiB), more than 4194304 poses for ld_complex_pair_contacts --
 * these three are checked before the list is read, so an absurd n is an error, not a crash -- and sets whose bit rows,
 * n x ceil(U / 32) words for U distinct keys over the list, would exceed 1 GiB.  n == 0 is LD_OK and sets *n_clusters = 0
 * (offsets[0] = 0, *total_out = 0).  Further device workspace: a bit a key of the span between the smallest and the
 * largest key (at most 528 MiB); per workgroup in flight the slot of ld_complex_contacts plus a bit a residue pair, at
 * most 1024 slots and 256 MiB (or one slot). */
/* offsets: n + 1 words, the keys of pose i are keys[offsets[i] .. offsets[i + 1]).  keys == NULL: offsets and the total
 * only; otherwise cap is the room in keys.  Any output may be NULL.  ld_complex_last_kernel_ms then reports this call. */
int ld_complex_pair_contacts(ld_complex *c, size_t n, const double *poses, size_t stride, double cutoff /* 5.0 */,
                             uint32_t *offsets /* n + 1 */, uint32_t *keys /* cap, or NULL */, size_t cap,
                             size_t *total_out);
/* The two steps in one call, the sets never leaving the device; the outputs equal ld_fcc_cluster's on
 * ld_complex_pair_contacts's sets word for word.  set_sizes and consensus may be NULL.  ld_complex_last_kernel_ms then
 * reports this call from its first launch to its last. */
int ld_complex_cluster_fcc(ld_complex *c, size_t n, const double *poses, size_t stride, const double *scoring,
                           double cutoff /* 5.0 */, double threshold /* 0.6 */, uint32_t min_size /* 1 */,
                           int32_t *cluster_of /* n */, int32_t *centres /* n */, uint32_t *n_clusters /* 1 */,
                           uint32_t *set_sizes /* n, or NULL */, uint64_t *consensus /* n, or NULL */);
/* The kernels on the caller's sets; no complex is needed.  common: c_ij, n x n, the diagonal s_i. */
int ld_fcc_common(size_t n, const uint32_t *offsets /* n + 1 */, const uint32_t *keys, uint32_t *common /* n x n */);
int ld_fcc_cluster(size_t n, const uint32_t *offsets /* n + 1 */, const uint32_t *keys, const double *scoring /* n */,
                   double threshold, uint32_t min_size, int32_t *cluster_of /* n */, int32_t *centres /* n */,
                   uint32_t *n_clusters /* 1 */, uint64_t *consensus /* n, or NULL */);
int ld_fcc_last_kernel_ms(double *ms_out); /* device time of the calling thread's last ld_fcc_common / ld_fcc_cluster (HIP events) */

/* Model quality: how close every pose is to a reference (bound) complex -- fnat, i-RMSD, L-RMSD, from which DockQ and
 * the CAPRI class follow by host arithmetic (lightdock-rust_amd/assess.py).  The rule is this library's own, modelled
 * on CAPRI / DockQ; no byte compatibility with any outside tool is claimed.
 *   Reference: two PDB files, receptor and ligand of the bound complex, read like the model's (ATOM/HETATM records in
 *     file order).  Both share one frame, which may be any frame; it need not be the model's.
 *   Matching: a model atom is matched when the reference file of its side has a record with the same chain (column
 *     22), sequence number (23-26), insertion code (27), residue name (18-20) and atom name (13-16), blanks trimmed;
 *     the first such record in file order wins.  Everything below is over matched atoms only, on both sides; all
 *     matched atoms count (hydrogens, hetero atoms, beads).
 *   Coordinates: model atoms posed as above, then the integer thousandths "%8.3f" prints; reference coordinates
 *     llrint(x * 1000).  So a pose's measures are those of the file ld_complex_write_pdb writes for it.
 *   Native contacts: C = llrint(contact_cutoff * 1000), 1 <= C <= 30000.  A pair (receptor residue i, ligand residue
 *     j; residues and indices of the MODEL, as under "Interface contacts") is native iff in the reference some matched
 *     atom of i and some matched atom of j have dx^2 + dy^2 + dz^2 <= C^2 in exact integers.  The list is sorted by
 *     (i, j).  Per pose, kept = the native pairs for which the same test holds in the model; fnat = kept / n_native.
 *   Fit atoms: matched atoms named N, CA, C, O or P.
 *   L-RMSD: the proper rotation and translation that best superimpose the model's receptor fit atoms on the
 *     reference's are applied to the model; L-RMSD is then the RMSD over the ligand's fit atoms.
 *   i-RMSD: an interface residue is a residue of either side with a matched atom within interface_cutoff (same
 *     integer test, same bounds) of a matched atom of the other side in the reference; i-RMSD is the RMSD of the
 *     fit atoms of the interface residues of both sides together after their own best superposition.
 *   Proper rotations only: a mirror image is not a fit.
 *   DockQ = (fnat + 1 / (1 + (iRMSD / 1.5)^2) + 1 / (1 + (LRMSD / 8.5)^2)) / 3.  CAPRI class, best first: high:
 *     fnat >= 0.5 and (L <= 1 or i <= 1); medium: fnat >= 0.3 and (L <= 5 or i <= 2); acceptable: fnat >= 0.1 and
 *     (L <= 10 or i <= 4); otherwise incorrect.
 *   Numerics: per superposition the sums  sum m, sum |m|^2, sum m r^T  (m model, r reference centred once on the
 *     integer-rounded centroid of its receptor fit atoms) are accumulated as integers, exact and order-free, so a
 *     pose's results are the same bits whatever the batch, its place in it or the chunking.  Only centring, Horn's
 *     symmetric 4 x 4, its largest eigenvalue and eigenvector (cyclic Jacobi) and the square roots are f64; a valid
 *     pose never gives NaN.  When the receptor's fit atoms are collinear the best rotation is not unique and L-RMSD
 *     is unspecified (finite); i-RMSD is still the optimum.
 * ld_complex_set_reference refuses with LD_ERR_INVALID, leaving the complex WITHOUT a reference: fewer than 3 receptor
 * fit atoms, no ligand fit atom, fewer than 3 interface fit atoms, no native pair, a cutoff out of bounds, a reference
 * atom beyond 2000 A of the centroid of its receptor fit atoms; a file that cannot be read is LD_ERR_IO.
 * ld_complex_assess refuses with LD_ERR_INVALID, nothing written: no reference set, non-finite poses, a zero
 * quaternion, stride < pose_len, a posed coordinate of a used atom (a fit atom or an atom of a residue of a native
 * pair) beyond +-2000 A.  Device workspace: one slot of used atoms x 16 B per workgroup in flight, at most 1024 slots,
 * and 320 B a pose of a chunk of 65536 poses; together within 256 MiB (or one slot). */
int ld_complex_set_reference(ld_complex *c, const char *ref_receptor_pdb, const char *ref_ligand_pdb,
                             double contact_cutoff /* 5.0 */, double interface_cutoff /* 10.0 */);
int ld_complex_reference_counts(const ld_complex *c, uint32_t *out /* 6: matched rec, matched lig, native pairs,
                                rec fit, lig fit, interface fit */);
int ld_complex_native_pairs(const ld_complex *c, uint32_t *pairs /* n_native x 2: rec residue, lig residue */);
/* Any output may be NULL; n == 0 is LD_OK.  ld_complex_last_kernel_ms then reports this call's kernels. */
int ld_complex_assess(ld_complex *c, size_t n, const double *poses, size_t stride,
                      uint32_t *kept /* n */, double *lrmsd /* n */, double *irmsd /* n */);

/* Solvent-accessible surface: for every pose, the surface of each molecule alone and in the complex, and so the area
 * the interface buries, per pose and per atom.  No tool of the reference tree computes a surface; the rule is this
 * library's own: Shrake-Rupley on integers, in thousandths of an angstrom as "%8.3f" prints a coordinate.
 *   Atoms that take part: every ATOM / HETATM record of the two files, in file order, except element H or D and
 *     residues named MMB (membrane beads).  An excluded atom neither has a surface nor covers anyone's.  The element is
 *     columns 77-78, trimmed and upper-cased; if the record is too short for them or the field is blank, the first
 *     alphabetic character of columns 13-16.
 *   Radii in thousandths: C 1700, N 1550, O 1520, F 1470, P 1800, S 1800, CL 1750, SE 1900, BR 1850, I 1980, any other
 *     element 1800; an atom that takes no part reports 0.
 *   Probe: 0 <= probe <= 2.0 A, p = llrint(1000 * probe); the expanded radius of atom a is E_a = R_a + p.
 *   Directions: LD_SASA_POINTS golden-spiral directions as a fixed integer table (ld_sasa_directions),
 *     U[k] = rint(2^20 * (r cos(k g), r sin(k g), z)), z = 1 - (2k + 1) / 128, r = sqrt(1 - z^2), g = pi (3 - sqrt 5).
 *     No component is within 1e-3 of a rounding tie.
 *   Points: point k of atom a lies at c_a + ((E_a * U[k] + 2^19) >> 20), the product in 64 bits, the shift arithmetic,
 *     per component.  c_a is the posed atom (posing as above: the ligand's modes in the ligand frame) as the integer
 *     thousandths "%8.3f" prints, so the surface of a pose is that of the file ld_complex_write_pdb writes for it.
 *   Burial: point q of atom a is buried by atom b (b != a, b taking part) iff |q - c_b|^2 < E_b^2, strictly, in exact
 *     integers.
 *   Counts per atom: free_a, the points of a not buried by any atom of a's OWN molecule; bound_a, those not buried by
 *     any atom of either molecule.  bound_a <= free_a <= 128; both are 0 for an atom that takes no part.
 *   Sums per pose, four uint64 in this order: sum free_a E_a^2 and sum bound_a E_a^2 over the receptor, then the same
 *     two over the ligand.  An area in A^2 is sum * 4 pi / (128e6); the area a model buries is
 *     (s0 - s1 + s2 - s3) * 4 pi / (128e6).
 *   The directions are fixed in the run's frame and rounding follows posing, so the ligand's free counts change with
 *     the pose even without modes.  Every result is the same bits whatever the batch.
 * LD_ERR_INVALID, nothing written: a probe that is negative, above 2.0 or not finite; non-finite poses, a zero
 * quaternion, stride < pose_len; a posed coordinate of an atom that takes part beyond +-1.0e6 A; a complex in which no
 * atom of a side takes part; a side other than 0 / 1.  Device workspace: one slot of 36 B an atom that takes part per
 * workgroup in flight, at most 1024 slots and 256 MiB (or one slot); per-atom counts are produced in chunks of poses
 * within 256 MiB. */
#define LD_SASA_POINTS (128)
int ld_sasa_directions(int32_t *out /* LD_SASA_POINTS x 3 */); /* host only */
int ld_complex_sasa_radii(const ld_complex *c, int side, uint32_t *radii_out /* n_atoms of that side, thousandths */); /* host only */
/* Any output may be NULL; n == 0 is LD_OK.  ld_complex_last_kernel_ms then reports this call's device work. */
int ld_complex_sasa(ld_complex *c, size_t n, const double *poses, size_t stride, double probe /* 1.4 */,
                    uint64_t *sums /* n x 4 */, uint8_t *free_counts /* n x (n_rec + n_lig), receptor first, file order */,
                    uint8_t *bound_counts /* as free_counts */);

/* Collision cross-section: for every pose, the orientation-averaged projected area of the receptor, of the posed ligand or
 * of the complex -- the number an ion-mobility measurement of native mass spectrometry gives -- by the projection
 * approximation (PA).  No tool of the reference tree computes one; the rule is this library's own: discs on a lattice, all
 * integers, in thousandths of an angstrom as "%8.3f" prints a coordinate.
 *   Atoms and radii: exactly the surface's (above): the atoms that take part and their radii R_a are those of
 *     ld_complex_sasa_radii; H, D and MMB residues take no part.  Probe: 0 <= probe <= 2.0 A, p = llrint(1000 * probe),
 *     E_a = R_a + p.  The default probe of 1.0 A is a parameter of the method, not a measurement.
 *   Selection `what`: 0 the receptor alone, 1 the ligand alone (posed), 2 the complex.
 *   Views: LD_CCS_VIEWS = 64 directions, the upper hemisphere of the surface's spiral (a projection along u and along -u
 *     has the same area).  For v = 0 .. 63: z = 1 - (2v + 1) / 128, r = sqrt(1 - z^2), g = pi (3 - sqrt 5), c = cos(v g),
 *     s = sin(v g); the in-plane axes e1 = (-s, c, 0), e2 = (-z c, -z s, r); the integer frames A[v] = rint(2^20 * e1),
 *     B[v] = rint(2^20 * e2), a fixed table (ld_ccs_frames).  No component is within 1e-3 of a rounding tie.
 *   Projection of a posed atom c_a (posing as above; the integer thousandths ld_complex_write_pdb prints):
 *     a = (A[v] . c_a + 2^19) >> 20 and b = (B[v] . c_a + 2^19) >> 20, the dot products in 64 bits, the shifts arithmetic.
 *   Lattice: h = llrint(1000 * cell), 100 <= h <= 2000, default 500.  The lattice points of every view are (i h, j h) for
 *     all integers i, j: anchored at the frame's origin, so the lattice does not depend on the batch.  Point (i, j) is
 *     covered by atom a iff (i h - a)^2 + (j h - b)^2 <= E_a^2, inclusively, in exact integers.  N[pose][v] is the number
 *     of lattice points covered by at least one selected atom.
 *   Outputs: counts, n x 64 uint32, N itself; sums[pose] = sum over v of N[pose][v], uint64.  The area of a view in A^2 is
 *     N h^2 / 1e6 and CCS_PA = sums h^2 / (64e6).
 *   Bounds: a posed coordinate of a selected atom beyond +-1.0e6 A refuses the call, as the surface does.  In any view,
 *     with I and J the counts of lattice columns and rows that the box [min(a - E), max(a + E)] x [min(b - E), max(b + E)]
 *     of the selected atoms touches, I * J > 2^28 refuses the call; a count then fits 32 bits.
 *   Every result is the same bits whatever the batch, a pose's place in it, the slot count, or how the plane is cut into
 *     pieces; without receptor modes the receptor's discs are rasterised once a call, to the same bits.
 * LD_ERR_INVALID, nothing written: a probe or a cell out of range or not finite; `what` not in 0 .. 2; non-finite poses, a
 * zero quaternion, stride < pose_len; no selected atom takes part; the two bounds.  Device workspace: one slot of 32 B a
 * selected atom per workgroup in flight, at most 1024 slots and 256 MiB (or one slot); up to 64 MiB for a rigid receptor's
 * bitmaps; the counts leave in chunks of poses within 256 MiB. */
#define LD_CCS_VIEWS (64)
int ld_ccs_frames(int32_t *out /* LD_CCS_VIEWS x 2 x 3: A then B */); /* host only */
/* Any output may be NULL; n == 0 is LD_OK.  ld_complex_last_kernel_ms then reports this call's device work. */
int ld_complex_ccs(ld_complex *c, size_t n, const double *poses, size_t stride, int what, double probe /* 1.0 */,
                   double cell /* 0.5 */, uint32_t *counts /* n x LD_CCS_VIEWS */, uint64_t *sums /* n */);

/* Cross-links: for every pose and every link of a list (a, b) of atoms that a chemical cross-linker of known length has
 * joined (XL-MS), the straight distance of the two atoms and the length of the shortest path between them that stays in the
 * solvent -- the solvent-accessible surface distance (SASD) of Xwalk and Jwalk.  No tool of the reference tree computes a
 * cross-link distance; the rule is this library's own: shortest paths on a lattice, all integers, in thousandths of an
 * angstrom as "%8.3f" prints a coordinate.
 *   Posed atoms: c_x, posing and rounding as above (the ligand's modes in the ligand frame; the integer thousandths
 *     ld_complex_write_pdb prints).
 *   Links: L pairs (a, b) of complex atom indices -- receptor atoms first, then ligand atoms, in file order --
 *     1 <= L <= 4096.  An anchor may be any atom, a hydrogen or an atom that takes no part in the surface too; both anchors
 *     may lie on the same molecule; a == b is allowed.
 *   Straight distance: straight2[pose][l] = |c_a - c_b|^2, uint64, exact.
 *   Blockers: the atoms that take part in the surface and their radii R_x, exactly those of ld_complex_sasa_radii.  Probe:
 *     0 <= probe <= 2.0 A, p = llrint(1000 * probe), E_x = R_x + p.  The default 0.0 is a parameter of the method.
 *   Lattice: h = llrint(1000 * cell), 500 <= h <= 2000, default 1000.  The nodes are (i h, j h, k h) for all integers i, j,
 *     k: anchored at the frame's origin, so the lattice depends neither on the batch nor on the link.  A node q is blocked
 *     iff some blocker x has |q - c_x|^2 < E_x^2, strictly, in exact integers; otherwise it is free.
 *   Moves: from a free node to any free node among its 26 neighbours, of weight w1 = h along an axis, w2 = isqrt(2 h^2)
 *     across a face, w3 = isqrt(3 h^2) across a cube; isqrt is the floor of the square root, in exact integers.
 *   Reach: rho = llrint(1000 * reach), 1 <= rho <= 6000, default 3000.  The doors of an anchor a are the free nodes q with
 *     |q - c_a|^2 <= rho^2, inclusively; the hop from a to its door q is s_a(q) = isqrt(|q - c_a|^2).  Atoms do not block a
 *     hop: it stands for the side chain.
 *   Path: D(a, b) = the minimum over the doors q of a, the doors q' of b and the lattice paths from q to q' over free nodes
 *     of s_a(q) + (the sum of the moves' weights) + s_b(q').  A path of no moves is allowed (q = q').
 *   Cap: M = llrint(1000 * max_length), h <= M <= 60000, default 35000, and floor(M / h) <= 80: a search looks at no more
 *     than 162^3 nodes (161^3 where h divides M).
 *   Outputs: path[pose][l] = D as a uint32 if D <= M, else LD_XLINK_NO_PATH: an anchor without a door, an anchor sealed in
 *     by blocked nodes, or a path longer than M.
 *   D is symmetric in (a, b).  Every result is the same bits whatever the batch, a pose's place in it, the slot count, the
 *     order or the repetition of the links, or the schedule of the search: on integer nodes with integer weights the field of
 *     shortest distances is a unique fixed point.
 *   A path over the 26 neighbours of a lattice overestimates the true geodesic by a few percent, most in the directions
 *     farthest from an axis, a face diagonal and a cube diagonal -- the approximation Xwalk and Jwalk make.
 * LD_ERR_INVALID, nothing written: a probe, a cell, a reach or a max_length out of range or not finite; n_links 0 or above
 * 4096; an atom index >= the number of atoms of the complex; non-finite poses, a zero quaternion, stride < pose_len; a posed
 * anchor beyond +-1.0e6 A, or, when `path` is asked for, a posed blocker beyond it; `path` asked for in a complex of which
 * no atom takes part.  Device workspace: with `path` one slot per workgroup in flight -- 16 B a blocker, 2 B a node of
 * (2 floor(M / h) + 4)^3 at most and, beyond 48 KiB of them, its bits -- at most 512 slots and 256 MiB (or one slot); without
 * `path` none.  The outputs leave in chunks of poses within 256 MiB. */
#define LD_XLINK_NO_PATH (0xFFFFFFFFu)
/* Either output may be NULL; n == 0 is LD_OK.  ld_complex_last_kernel_ms then reports this call's device work. */
int ld_complex_crosslinks(ld_complex *c, size_t n, const double *poses, size_t stride, size_t n_links,
                          const uint32_t *links /* n_links x 2 */, double probe /* 0.0 */, double cell /* 1.0 */,
                          double reach /* 3.0 */, double max_length /* 35.0 */, uint64_t *straight2 /* n x n_links */,
                          uint32_t *path /* n x n_links */);

/* Small-angle scattering: for every pose, the histogram of all pair distances by pair class and, from it, the SAXS
 * profile I(q) by the Debye formula, to be fitted to an experimental curve.  No tool of the reference tree computes a
 * profile; the rule is this library's own.  The profile is "vacuum minus excluded volume" of the atoms in the files: no
 * implicit hydrogens and no hydration layer are modelled; hydrogens take part when the files hold them.
 *   Atoms that take part: every ATOM / HETATM record of the two files, in file order, except residues named MMB (membrane
 *     beads).  The element is read by the surface's rule (columns 77-78, trimmed and upper-cased, else the first
 *     alphabetic character of columns 13-16).  Six classes: H (also D) = 0, C = 1, N = 2, O = 3, P = 4, S = 5.  An atom of
 *     any other element, or of an MMB residue, takes no part and reports class 255.  At most 65536 atoms of a complex may
 *     take part, so that a bin count fits 32 bits.
 *   Pair class of classes e <= e': c = 6 e - e (e - 1) / 2 + (e' - e), 21 values: (0,0) .. (0,5) are 0 .. 5, (5,5) is 20.
 *   Histogram: the posed atoms are the integer thousandths ld_complex_write_pdb prints (posing and rounding as above).
 *     For every unordered pair a < b of atoms that take part, of either molecule, d^2 = |c_a - c_b|^2 in exact integers
 *     (a per-axis |d| is clamped at 2^22 - 1, above 1024 x 2000: a clamped pair is beyond the last bin anyway).  The pair
 *     falls in bin k, the largest integer with (k w)^2 <= d^2; w is the bin width in thousandths, 100 <= w <= 2000.
 *     counts[pose][c][k] is the number of such pairs, 1 <= bins <= 1024.  A pair with k >= bins refuses the call.
 *     Rounding follows posing, so the ligand's own pairs change with the pose even without modes; the receptor's own
 *     pairs do not when the receptor has no modes.
 *   Form factors at q in 1 / A, u = (q / 4 pi)^2:  f_e(q) = sum_{k=1..4} a_k exp(-b_k u) + c - rho0 V_e exp(-q^2 V_e^(2/3) / (4 pi)),
 *     rho0 = 0.334, with Cromer-Mann coefficients and Fraser's displaced volumes (A^3):
 *            a1        a2        a3        a4        b1        b2        b3        b4        c         V
 *       H    0.489918  0.262003  0.196767  0.049879  20.6593   7.74039   49.5519   2.20159   0.001305  5.15
 *       C    2.31000   1.02000   1.58860   0.865000  20.8439   10.2075   0.568700  51.6512   0.215600  16.44
 *       N    12.2126   3.13220   2.01250   1.16630   0.005700  9.89330   28.9975   0.582600  -11.529   2.49
 *       O    3.04850   2.28680   1.54630   0.867000  13.2771   5.70110   0.323900  32.9089   0.250800  9.13
 *       P    6.43450   4.17910   1.78000   1.49080   1.90670   27.1570   0.526000  68.1645   1.11490   5.73
 *       S    6.90530   5.20340   1.43790   1.58630   1.46790   22.2151   0.253600  56.1720   0.866900  19.86
 *   Debye sum: r_k = (k + 0.5) w / 1000 A, s(x) = 1 if x == 0 else sin(x) / x.  For each pose and q_j:
 *       G_c = sum over k ascending of (double)counts[c][k] * s(q_j r_k), from 0
 *       I(q_j) = S_j, then + F_{j,c} * G_c for c ascending
 *       S_j = sum over e ascending of (double)N_e * (f_e(q_j) * f_e(q_j)), from 0; N_e the atoms of class e
 *       F_{j,c} = (2 f_e(q_j)) * f_e'(q_j)
 *     Every product and sum is a separately rounded f64 operation, no fma, no reassociation.  f, s, S and F are made on
 *     the HOST with libm and handed to the kernel; the device evaluates no sin or exp.  So an intensity is the same bits
 *     whatever the batch, and a loop over k on ld_saxs_form_factors and ld_saxs_sinc restates it exactly.
 *     1 <= n_q <= 1024, 0 <= q <= 1.0, finite.
 *   Fit, per pose, sums sequential over j from 0:
 *       scale = (sum_j I_exp I / sigma^2) / (sum_j I I / sigma^2), a term being (x * I) / (sigma * sigma)
 *       chi2 = (sum_j ((I_exp - scale I) / sigma)^2) / n_q
 * LD_ERR_INVALID, nothing written: width, bins, n_q or q out of range; non-finite poses, a zero quaternion,
 * stride < pose_len; a pair beyond the last bin; a posed coordinate of an atom that takes part beyond +-1.0e6 A; no atom
 * taking part, or more than 65536; a side other than 0 / 1; a sigma that is not finite and > 0, a non-finite I_exp or
 * intensity, a zero denominator of the scale.  n == 0 is LD_OK.  Device workspace: the counts are produced in chunks of
 * poses, 84 B a bin and 16 B an atom that takes part a pose, within 256 MiB (or one pose). */
#define LD_SAXS_CLASSES (6)
#define LD_SAXS_PAIR_CLASSES (21)
int ld_complex_saxs_classes(const ld_complex *c, int side, uint8_t *class_out /* n_atoms of that side; 255: no part */); /* host only */
int ld_saxs_form_factors(const double *q, size_t n_q, double *f_out /* n_q x 6 */); /* host only */
int ld_saxs_sinc(const double *q, size_t n_q, uint32_t width, size_t bins, double *s_out /* n_q x bins */); /* host only */
/* counts may be NULL.  ld_complex_last_kernel_ms then reports this call's device work. */
int ld_complex_distance_histogram(ld_complex *c, size_t n, const double *poses, size_t stride, uint32_t width /* 500 */,
                                  size_t bins, uint32_t *counts /* n x 21 x bins */);
/* The Debye sum on the caller's counts (GPU; host arrays in and out, like ld_fcc_common); class_atoms: N_e. */
int ld_saxs_debye(size_t n, const uint32_t *counts /* n x 21 x bins */, uint32_t width, size_t bins,
                  const uint32_t class_atoms[6], const double *q, size_t n_q, double *intensity /* n x n_q */);
/* Histogram and Debye sum in one call, the counts staying on the device unless asked for.  Either output may be NULL.
 * ld_complex_last_kernel_ms then reports this call's device work: posing, histogram and Debye sum of every chunk. */
int ld_complex_saxs(ld_complex *c, size_t n, const double *poses, size_t stride, uint32_t width /* 500 */, size_t bins,
                    const double *q, size_t n_q, double *intensity /* n x n_q */, uint32_t *counts /* n x 21 x bins, or NULL */);
/* Poses a chunk of counts in the two calls above; 0 (the default): as many as 256 MiB hold.  Results do not depend on it. */
int ld_complex_saxs_chunk(ld_complex *c, size_t poses);
int ld_saxs_fit(size_t n, size_t n_q, const double *intensity /* n x n_q */, const double *i_exp /* n_q */,
                const double *sigma /* n_q */, double *scale_out /* n, or NULL */, double *chi2_out /* n, or NULL */); /* host only */

/* Density fit: for every pose, the density its atoms would show in a cryo-EM map at a given resolution, and the exact
 * sums from which its correlation with the map follows.  No tool of the reference tree reads a volume; the rule is this
 * library's own, modelled on Chimera's molmap and "fit in map".  Everything on the device is an integer, so a pose's
 * words are the same whatever the batch, its place in it or the chunk, and a numpy restatement gives the same words.
 *   Map: nx x ny x nz voxels, x fastest; the centre of voxel (i, j, k) is origin + (i hx, j hy, k hz), all in integer
 *     thousandths of an A in the run's frame (that of lightdock_<rec>.pdb).  1 <= n <= 1024 an axis, at most 2^24 voxels,
 *     200 <= h <= 20000, |origin| <= 10^9.  Values arrive as float.  A value below threshold (>= 0, default 0: negative
 *     density counts as none) becomes 0; the quantised voxel is E = rint(rho' * (32767.0 / max rho')) in double, so
 *     0 <= E <= 32767.  A map with a value that is not finite, or with no positive value left, is refused.  Constants of
 *     a map: N voxels, S_e = sum E, S_ee = sum E^2.
 *   Atoms: posed and rounded as under "Small-angle scattering" above, and exactly its atoms take part (class != 255).
 *     The weight w of an atom is the atomic number of its class: H 1, C 6, N 7, O 8, P 15, S 16.  At most 65536 atoms.
 *   Kernel table, made by the HOST with libm from sigma in thousandths, 300 <= sigma <= 15000 (a tool passes
 *     sigma = rint(225 * resolution), which is resolution / (pi sqrt 2) to three digits):
 *       two = 2 sigma^2;  L = floor(two * ln 510) + 1, the first d^2 at which 255 exp(-d^2 / two) rounds to 0;
 *       s = the smallest shift with ((L - 1) >> s) + 1 <= 4096;  T = ((L - 1) >> s) + 1;
 *       K[t] = rint(255 * exp(-(((double)t + 0.5) * (double)(1 << s)) / (double)two)),  t < T.
 *     An atom at the exact integer squared distance d^2 from a voxel's centre adds w * K[d^2 >> s] to that voxel when
 *     d^2 < T << s, and nothing otherwise.  A voxel outside the grid receives nothing: a support that leaves the map is
 *     clipped.  The device evaluates no exp.  T << s is below 2^32 for every sigma (2676 << 20 at 15000); d^2 itself may
 *     pass 32 bits: an axis difference above isqrt((T << s) - 1) decides alone, the rest is summed in 64 bits.
 *     A call is refused when isqrt(T << s) > 16 * min(hx, hy, hz): the map is far finer than the table needs (bin it).
 *   Per pose, with rho_s(v) the simulated voxel, exact integers:
 *       s = sum rho_s;  ss = sum rho_s^2;  se = sum rho_s E;  inside_sum = sum of rho_s over the voxels with E > 0;
 *       outside = the atoms taking part that lie in no voxel's cell: 2 (x - X[0]) < -hx or 2 (x - X[nx - 1]) >= hx, and
 *       likewise on y and z.
 *   Widths: a uint32 voxel cannot wrap (65536 * 16 * 255 < 2^32).  A pose with a voxel >= 2^24 or s >= 2^40 refuses the
 *     call.  Below those limits ss < 2^24 * s < 2^64 and se <= 32767 * s < 2^55.
 *   Scores, made by the host in one order of operations; every integer is converted once to double with correct
 *     rounding, products of the 64-bit sums are taken in 128 bits:
 *       cc = (double)se / (sqrt((double)ss) * sqrt((double)S_ee)), 0 when ss = 0;
 *       A = N se - s S_e, B = N ss - s^2, C = N S_ee - S_e^2;
 *       ccm = (double)A / (sqrt((double)B) * sqrt((double)C)), 0 when B = 0 or C = 0;
 *       inside = (double)inside_sum / (double)s, 0 when s = 0.
 *   Without receptor modes the receptor's density is the same for every pose: it is deposited once a call and a pose
 *     visits only the bricks of 16 x 16 x 4 voxels its ligand's supports reach; with receptor modes every pose deposits all its
 *     atoms.  The words are the same either way.
 * LD_ERR_INVALID, nothing written: a map, sigma or threshold out of range; a support wider than 16 voxels; non-finite
 * poses, a zero quaternion, stride < pose_len; a posed coordinate of an atom that takes part beyond +-1.0e6 A; a voxel
 * >= 2^24 or s >= 2^40; no atom taking part, or more than 65536; more than 256 MiB of simulated voxels.  n == 0 is LD_OK.
 * Device workspace: chunks of poses, 16 B an atom and 8 B a brick a pose (and 4 B a voxel when voxels are asked for),
 * within 256 MiB (or one pose); 4 B a voxel for the receptor's grid. */
typedef struct ld_density ld_density;
typedef struct ld_density_sums {
    uint64_t s;
    uint64_t ss;
    uint64_t se;
    uint64_t inside_sum;
    uint32_t outside;
    uint32_t reserved; /* 0 */
} ld_density_sums;
/* NULL (ld_last_error) on a refusal.  Host only: the voxels reach the device with the first fit. */
ld_density *ld_density_create(const float *rho /* nx x ny x nz, x fastest */, const uint32_t n[3], const int32_t origin[3],
                              const uint32_t step[3], double threshold);
void ld_density_destroy(ld_density *d);
/* Any output may be NULL.  scale: 32767.0 / max rho'. */
int ld_density_info(const ld_density *d, uint64_t *n_voxels, uint64_t *s_e, uint64_t *s_ee, double *scale); /* host only */
int ld_density_voxels(const ld_density *d, uint32_t *voxels_out /* N: E */); /* host only */
/* table_out == NULL asks for the length and the shift only. */
int ld_density_kernel(uint32_t sigma, uint32_t *table_out /* T, or NULL */, uint32_t *length_out, uint32_t *shift_out); /* host only */
/* ld_complex_last_kernel_ms then reports this call's device work. */
int ld_complex_density_fit(ld_complex *c, ld_density *d, size_t n, const double *poses, size_t stride, uint32_t sigma,
                           ld_density_sums *out /* n */);
/* The simulated voxels themselves, x fastest; refused above 256 MiB of output. */
int ld_complex_simulate_density(ld_complex *c, ld_density *d, size_t n, const double *poses, size_t stride, uint32_t sigma,
                                uint32_t *grid /* n x N */);
/* Any output may be NULL. */
int ld_density_scores(const ld_density *d, size_t n, const ld_density_sums *sums /* n */, double *cc /* n */, double *ccm /* n */,
                      double *inside /* n */); /* host only */
/* Poses a chunk in the two ld_complex_ calls above; 0 (the default): as many as 256 MiB hold.  Results do not depend on it. */
int ld_complex_density_chunk(ld_complex *c, size_t poses);

/* ------------------------------------------------------------------------------------
 * Normal modes: the rec_nm.npy / lig_nm.npy a run with `use_anm: true` reads
 * (src/bin/lightdock-rust.rs:216-254 is the consumer; the reference tree cannot produce them,
 * lightdock3_setup.py asks ProDy).  The rule is ProDy's anisotropic network model on one node per
 * residue, extended to all atoms as LightDock does; it reproduces the mode files under
 * tests/golden up to each mode's sign.
 *   Atoms and residues: the ATOM / HETATM records in file order; residues as under "Interface
 *     contacts" above.
 *   Node of a residue: its first atom named CA, else its first atom named C4'.  A residue with
 *     neither is refused (LD_ERR_INVALID, the residue id in ld_last_error()).
 *   Hessian, 3m x 3m for m nodes, spring constant 1: for i != j with 0 < d^2 <= cutoff^2 the
 *     off-diagonal 3 x 3 block is -d d^T / d^2, d = x_j - x_i; a diagonal block is minus the sum of
 *     its row's off-diagonal blocks, j ascending.
 *   Modes: eigenpairs ascending; the six smallest are rigid-body motions; the modes are the 7th to
 *     the (6 + n_modes)-th.  Sign: the component of largest magnitude of the node eigenvector (the
 *     lowest index on a tie) is positive (ProDy's sign is LAPACK's accident).
 *   Extension: every atom takes its residue's node vector; each mode is then divided by its
 *     Euclidean norm over all atoms x 3.
 *   Amplitude (this library's own option, the expectation form of ProDy's sampleModes scale; only
 *     the DIRECTION of a mode is claimed to equal a setup made with anm_rec_rmsd / anm_seed): with
 *     rmsd > 0 mode k is further multiplied by rmsd sqrt(atoms) / sqrt(sum_j 1 / lambda_j) /
 *     sqrt(lambda_k), j over the n_modes modes.
 *   Solver: parallel one-sided Jacobi on the device, f64, to |a_p . a_q| <= 2^-50 |a_p| |a_q| for
 *     every column pair; all sums in a fixed order, so the same input gives the same bits.
 * LD_ERR_INVALID, nothing written: a null argument, n_modes == 0 or > 128, more than 4096 nodes,
 * 3m < 6 + n_modes, a cutoff that is not positive and finite, a negative or non-finite rmsd, a
 * non-finite coordinate, a seventh eigenvalue below 1e-6 (a floppy, collinear or disconnected
 * network).  LD_ERR_INTERNAL, nothing written: no convergence within 40 sweeps.  A file that
 * cannot be read is LD_ERR_IO.  Device memory: two matrices of (3m)^2 doubles for the call.
 * ---------------------------------------------------------------------------------- */
/* Host only.  node_atom_out: n_residues record indices (file order), or NULL to ask for the count alone. */
int ld_anm_nodes(const char *pdb_path, uint32_t *node_atom_out /* n_residues or NULL */, size_t *n_residues_out);
/* The core on raw coordinates; the modes of the nodes themselves, each of norm 1. */
int ld_anm_modes_xyz(const double *node_xyz /* n_nodes x 3 */, size_t n_nodes, size_t n_modes, double cutoff /* 15.0 */,
                     double *node_modes_out /* n_modes x n_nodes x 3 */, double *eigenvalues_out /* n_modes or NULL */);
/* From a PDB file to what rec_nm.npy holds.  rmsd == 0: unit modes. */
int ld_anm_modes(const char *pdb_path, size_t n_modes, double cutoff /* 15.0 */, double rmsd /* 0.0 */,
                 double *modes_out /* n_modes x atoms x 3, file order */, double *eigenvalues_out /* n_modes or NULL */);
/* The device work of this thread's last ld_anm_modes / ld_anm_modes_xyz that reached the device (HIP events, from the
 * first launch to the last, the host's reads of the sweeps' convergence word included). */
int ld_anm_last_kernel_ms(double *ms_out);

/* ------------------------------------------------------------------------------------
 * Preparing a run: the swarm centres and the start poses lightdock3_setup.py computes, so that a
 * run starts from its two PDB files alone (lightdock-rust_amd/prepare.py).  LightDock's own
 * placement (ProDy's surface selection, scipy's kmeans2) cannot be reproduced and is not claimed;
 * the rule is this library's own, modelled on it.  Every decision that picks a centre is exact
 * integer arithmetic on int32 thousandths of an angstrom, as "%8.3f" prints a coordinate of the
 * cleaned, centred files; |x| <= 2 000 000 or the call is refused.
 *   1. Distance D = isqrt(max_{i,j} |l_i - l_j|^2) / 4, floor both times, over the ligand's atoms
 *      with a radius > 0 under "Solvent-accessible surface" (ld_swarm_diameter2 gives the maximum).
 *   2. Shell candidates (ld_swarm_shell).  An atom b has a centre c_b and an extent E_b: R_b + D for
 *      a receptor atom with R_b > 0, 2000 + D for a bead (a residue named MMB), which is flagged.
 *      Lattice nodes are p = (i h, j h, k h), h the spacing; per axis i runs from
 *      floor((min_b c_b - E_max - h) / h) to ceil((max_b c_b + E_max + h) / h).  A node is a candidate
 *      iff |p - c_b|^2 >= E_b^2 for EVERY atom and bead and |p - c_b|^2 < (E_b + h)^2 for SOME atom
 *      that is no bead: beads keep centres out of the membrane and attract none.  Candidates are
 *      numbered in lexicographic (x, y, z) order.
 *   3. Centres (ld_swarm_centres): farthest-point sampling.  The first centre is the candidate of
 *      largest |p|^2; each next one is the candidate, not chosen yet, whose smallest squared distance to
 *      the chosen ones (its gap^2) is largest; ties go to the lowest index.  Sampling ends after
 *      max_centres, when every candidate is chosen, and, with cover > 0, before a centre (the first
 *      excepted) whose gap^2 <= cover^2.
 *   4. Restraint filter (prepare.py, host): with restraint residues on the receptor a centre is kept
 *      iff it is among the swarms_per_restraint nearest (squared distance on thousandths, ties by
 *      centre index) to some restraint residue's CA, else P, else first atom; the kept centres are
 *      renumbered in ascending order.
 *   5. Poses (ld_initial_poses, host).  Stream: ld_stdrng_key(seed); u64 number k is words 2 (k % 8),
 *      2 (k % 8) + 1 of ChaCha block k / 8.  Glowworm g of swarm s of a run of G glowworms reads the
 *      draws ((s G + g) << 16) + j, j = 0, 1, ..: a row depends on (seed, s, g) alone.
 *      u = (bits >> 11) 2^-53, v = 2 u - 1.  In this order:
 *        translation: triples (v1, v2, v3) until (v1^2 + v2^2) + v3^2 <= 1; t = centre + radius v.
 *        rotation, unless both sides have restraint points (Marsaglia): pairs until r1 = x1^2 + y1^2
 *          < 1, pairs until 0 < r2 = x2^2 + y2^2 < 1; q = (x1, y1, x2 s, y2 s), s = sqrt((1 - r1) / r2).
 *        rotation with restraint points on both sides: one draw picks the receptor's, floor(u n_rec),
 *          the next the ligand's; q is the shortest arc taking a = unit(l) to b = unit(r - t), l in the
 *          centred ligand frame: q = normalise(1 + a.b, a x b); when 1 + a.b < 1e-12, half a turn about
 *          a x e, e the coordinate axis of a's smallest absolute component (the lowest on a tie); a zero
 *          l or r - t gives the identity.
 *        mode extents: anm_rec + anm_lig standard normals by the polar method: pairs until 0 < s =
 *          v1^2 + v2^2 < 1, each giving v1 f, v2 f, f = sqrt(-2 ln s / s); a left-over one is discarded.
 *      Sums of squares add left to right, no operation is fused.
 *   Cleaned files (ld_prepare_pdb, host): the ATOM / HETATM records in file order; element H or D
 *      (the surface rule's element test), atoms named OXT and residues HOH / WAT are dropped unless
 *      kept by flag, MMB is kept; with t the thousandths llrint(1000 x) of the n kept atoms and S their
 *      sum per axis, a coordinate becomes floor((2 (t n - S) + n) / (2 n)), printed "%8.3f".
 * LD_ERR_INVALID, every output as it was: a null argument; a coordinate beyond +-2 000 000; no
 * atoms, an extent outside 1 .. 4 000 000, a spacing outside 1 .. 1 000 000; a lattice of more than
 * 2^28 nodes or more than 2^22 candidates (the message names the spacing); a cap below the count
 * (count_out then holds the count, which is all that is written); more than 2^22 points, max_centres
 * == 0, a negative cover; more than 2^20 atoms for the diameter.  Device memory for the call only.
 * ---------------------------------------------------------------------------------- */
int ld_swarm_diameter2(const int32_t *xyz /* n x 3 */, size_t n, uint64_t *d2_out);
/* nodes_out NULL: the count alone.  lattice_nodes_out (or NULL): the nodes tested. */
int ld_swarm_shell(const int32_t *atoms /* n x 4: x y z E */, const uint8_t *bead /* n flags, or NULL: none */, size_t n,
                   int32_t spacing /* 2000 */, int32_t *nodes_out /* cap x 3 or NULL */, size_t cap, size_t *count_out,
                   uint64_t *lattice_nodes_out);
/* index_out, gap2_out: min(max_centres, n) entries; gap2_out[k] is the value centre k was picked at, |p|^2 for the
 * first, its gap^2 for the others (non-increasing from the second).  n == 0 is LD_OK with *n_out = 0. */
int ld_swarm_centres(const int32_t *points /* n x 3 */, size_t n, size_t max_centres, int32_t cover /* 0: no cover rule */,
                     uint32_t *index_out, uint64_t *gap2_out, size_t *n_out);
/* Host only.  Rows first .. first + n - 1 of swarm `swarm`; rows_out: n x (7 + anm_rec + anm_lig); draws_out: the u64
 * draws each row consumed, or NULL.  LD_ERR_INVALID, nothing written: rows that are no glowworms of the run, more than
 * 2^24 swarms or glowworms or 4096 modes a side, a negative radius, a non-finite value. */
int ld_initial_poses(uint64_t seed, size_t glowworms, size_t swarm, size_t first, size_t n, const double centre[3],
                     double radius /* 10.0 */, const double *rec_points /* n_rec x 3 or NULL */, size_t n_rec,
                     const double *lig_points /* n_lig x 3 or NULL */, size_t n_lig, size_t anm_rec, size_t anm_lig,
                     double *rows_out, uint64_t *draws_out);
/* Host only.  keep_flags: 1 hydrogens, 2 OXT, 4 waters.  LD_ERR_IO: a file that cannot be read or written, a record
 * shorter than 54 columns; LD_ERR_INVALID: no atom kept, a centred coordinate that "%8.3f" cannot hold.  The output file
 * is written only when every record has passed. */
#define LD_KEEP_HYDROGENS (1)
#define LD_KEEP_OXT (2)
#define LD_KEEP_WATERS (4)
int ld_prepare_pdb(const char *in_path, const char *out_path, int keep_flags, size_t *atoms_out /* or NULL */,
                   double centre_out[3] /* the mean subtracted, A; or NULL */);
/* The device work of this thread's last ld_swarm_diameter2 / ld_swarm_shell / ld_swarm_centres that reached the device
 * (HIP events; for the centres from the first step's launch to the last, the host's reads of the stop word included). */
int ld_setup_last_kernel_ms(double *ms_out);

/* ------------------------------------------------------------------------------------
 * The reference command line (src/bin/lightdock-rust.rs:77-333) as a function:
 *   argv = { prog, setup.json, initial_positions_N.dat, steps, dfire|dna|pydock }
 * Same stdout lines, same files, same "usage errors return 0" behaviour.
 * ---------------------------------------------------------------------------------- */
int ld_cli_main(int argc, char **argv);

#ifdef __cplusplus
}
#endif
#endif /* LIGHTDOCK_HIP_H */
