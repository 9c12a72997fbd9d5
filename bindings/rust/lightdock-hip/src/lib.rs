//! Thin, safe wrapper over `include/lightdock_hip.h` shaped like lightdock-rust's own types:
//! `HipScore` is what `DFIRE::new` / `DNA::new` / `PYDOCK::new` return (`Box<dyn Score>`,
//! lightdock-rust src/scoring.rs:11-19), `HipGso` is `GSO` (src/lib.rs:21-58) for a batch of swarms.
//!
//! The `Score` trait and `Quaternion` live in the lightdock crate; to keep this crate free of a
//! dependency cycle the trait impl is written against a local mirror and re-implemented in one
//! line inside lightdock-rust (Level 1).
use std::ffi::{CStr, CString};
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
pub struct LdMolecule {
    pub n_atoms: usize,
    pub coordinates: *const f64,
    pub dfire_types: *const u32,
    pub ele_charges: *const f64,
    pub vdw_charges: *const f64,
    pub vdw_radii: *const f64,
    pub n_membrane: usize,
    pub membrane: *const u32,
    pub n_restraint_groups: usize,
    pub restraint_offsets: *const u32,
    pub restraint_atoms: *const u32,
    pub num_anm: usize,
    pub nmodes: *const f64,
}

#[repr(C)]
pub struct LdScorerDesc {
    pub method: c_int, // 0 DFIRE, 1 DNA, 2 PYDOCK
    pub use_anm: c_int,
    pub receptor: LdMolecule,
    pub ligand: LdMolecule,
    pub potential: *const f64,
}

/// `ld_energy_terms`: the terms of one pose's energy (include/lightdock_hip.h, "Energy decomposition").
#[allow(non_camel_case_types)]
#[derive(Clone, Copy, Default)]
#[repr(C)]
pub struct ld_energy_terms {
    pub pair: [f64; 2],
    pub score: f64,
    pub rec_restraints: f64,
    pub lig_restraints: f64,
    pub membrane: f64,
    pub energy: f64,
    pub pairs: u32,
    pub rec_interface: u32,
    pub lig_interface: u32,
    pub reserved: u32,
}

/// `ld_group_energies`: the groups of one side and where their rows go; any pointer may be null.
#[allow(non_camel_case_types)]
#[repr(C)]
pub struct ld_group_energies {
    pub group_of_atom: *const u32,
    pub n_groups: usize,
    pub sums: *mut f64,
    pub pairs: *mut u32,
    pub interface_atoms: *mut u32,
}

pub const LD_GROUP_NONE: u32 = 0xffff_ffff;

/// `ld_refine_history`: j* on an accept, -1 halved, -2 frozen in this iteration, -3 not evaluated
/// (include/lightdock_hip.h, "Local refinement").
#[allow(non_camel_case_types)]
pub type ld_refine_history = i16;

/// `ld_refine_options`: the iterations, the step halvings a pose may take and the three start steps.
#[allow(non_camel_case_types)]
#[derive(Clone, Copy)]
#[repr(C)]
pub struct ld_refine_options {
    pub iterations: u32,
    pub max_halvings: u32,
    pub trans_step: f64,
    pub rot_step: f64,
    pub nm_step: f64,
    pub slice_poses: u32,
    pub reserved: u32,
}

/// `ld_refine_stats`: what the refinement made of one pose.
#[allow(non_camel_case_types)]
#[derive(Clone, Copy, Default)]
#[repr(C)]
pub struct ld_refine_stats {
    pub energy_before: f64,
    pub energy_after: f64,
    pub accepted: u32,
    pub halvings: u32,
    pub evaluations: u32,
    pub frozen: u32,
}

/// `ld_refine_state`: the per-pose arrays the two kernel entry points take.
#[allow(non_camel_case_types)]
#[repr(C)]
pub struct ld_refine_state {
    pub energy: *mut f64,
    pub trans_step: *mut f64,
    pub rot_cos: *mut f64,
    pub rot_sin: *mut f64,
    pub nm_step: *mut f64,
    pub halvings: *mut u32,
    pub accepted: *mut u32,
    pub evaluations: *mut u32,
    pub frozen: *mut u8,
}

/// `ld_complex`: the opaque handle of the analysis half of a run (include/lightdock_hip.h, "Analysis of a finished run").
#[allow(non_camel_case_types)]
#[repr(C)]
pub struct ld_complex {
    _private: [u8; 0],
}

/// `ld_density`: the opaque handle of a quantised density map (include/lightdock_hip.h, "Density fit").
#[allow(non_camel_case_types)]
#[repr(C)]
pub struct ld_density {
    _private: [u8; 0],
}

/// `ld_density_sums`: the exact sums of one pose's simulated density against a map.
#[allow(non_camel_case_types)]
#[repr(C)]
pub struct ld_density_sums {
    pub s: u64,
    pub ss: u64,
    pub se: u64,
    pub inside_sum: u64,
    pub outside: u32,
    pub reserved: u32,
}

pub const LD_SASA_POINTS: usize = 128;

// The decomposition, refinement and residue entry points (ld_scorer_decompose*, ld_scorer_refine*, ld_refine_*, ld_model_*) are declared only: no wrapper uses them yet.
#[allow(dead_code)]
extern "C" {
    fn ld_init(device: c_int) -> c_int;
    fn ld_last_error() -> *const c_char;
    fn ld_scorer_create(desc: *const LdScorerDesc) -> *mut c_void;
    fn ld_scorer_destroy(s: *mut c_void);
    fn ld_scorer_pose_len(s: *const c_void) -> usize;
    fn ld_scorer_energy(s: *mut c_void, t: *const f64, q_wxyz: *const f64, rec_nm: *const f64, lig_nm: *const f64,
                        out: *mut f64) -> c_int;
    fn ld_scorer_energy_batch(s: *mut c_void, n: usize, poses: *const f64, stride: usize, out: *mut f64) -> c_int;
    fn ld_scorer_decompose(s: *mut c_void, n: usize, poses: *const f64, stride: usize, terms_out: *mut ld_energy_terms,
                           receptor: *const ld_group_energies, ligand: *const ld_group_energies) -> c_int;
    fn ld_scorer_decompose_info(s: *const c_void, slice_poses_out: *mut usize, last_kernel_ms_out: *mut f64) -> c_int;
    fn ld_scorer_refine(s: *mut c_void, opts: *const ld_refine_options, n: usize, poses: *const f64, stride: usize,
                        poses_out: *mut f64, stats_out: *mut ld_refine_stats, history_out: *mut ld_refine_history) -> c_int;
    fn ld_scorer_refine_info(s: *const c_void, trials_out: *mut usize, slice_poses_out: *mut usize, last_kernel_ms_out: *mut f64,
                             evaluations_out: *mut u64) -> c_int;
    fn ld_refine_plan(pose_len: usize, n: usize, stride: usize, iterations: u32, slice_poses: u32, trials_out: *mut usize,
                      slice_poses_out: *mut usize, workspace_bytes_out: *mut usize) -> c_int;
    fn ld_refine_trials(n: usize, pose_len: usize, poses: *const f64, stride: usize, state: *const ld_refine_state,
                        trials: *mut f64, trial_stride: usize, active_out: *mut u8) -> c_int;
    fn ld_refine_select(n: usize, pose_len: usize, poses: *mut f64, stride: usize, state: *const ld_refine_state,
                        energies: *const f64, max_halvings: u32, history_out: *mut ld_refine_history) -> c_int;
    fn ld_model_from_pdb(method: c_int, pdb_path: *const c_char, active: *const *const c_char, n_active: usize,
                         passive: *const *const c_char, n_passive: usize, nmodes: *const f64, nmodes_len: usize, num_anm: usize) -> *mut c_void;
    fn ld_model_view(m: *const c_void, out: *mut LdMolecule) -> c_int;
    fn ld_model_destroy(m: *mut c_void);
    fn ld_model_num_residues(m: *const c_void) -> usize;
    fn ld_model_residue_id(m: *const c_void, index: usize, buf: *mut c_char, buf_len: usize) -> c_int;
    fn ld_model_residue_of_atom(m: *const c_void, out: *mut u32) -> c_int;
    fn ld_gso_create(s: *mut c_void, n_swarms: usize, n_glowworms: usize, positions: *const f64, seeds: *const u64) -> *mut c_void;
    fn ld_gso_destroy(g: *mut c_void);
    fn ld_gso_run(g: *mut c_void, steps: u32) -> c_int;
    fn ld_gso_save(g: *mut c_void, swarm: usize, step: u32, dir: *const c_char) -> c_int;
    fn ld_gso_save_many(g: *mut c_void, n: usize, swarms: *const usize, dirs: *const *const c_char, step: u32) -> c_int;
    // Normal modes (include/lightdock_hip.h, "Normal modes"): what src/bin/lightdock-rust.rs:216-254 reads as rec_nm.npy / lig_nm.npy
    pub fn ld_anm_nodes(pdb_path: *const c_char, node_atom_out: *mut u32, n_residues_out: *mut usize) -> c_int;
    pub fn ld_anm_modes_xyz(node_xyz: *const f64, n_nodes: usize, n_modes: usize, cutoff: f64, node_modes_out: *mut f64,
                            eigenvalues_out: *mut f64) -> c_int;
    pub fn ld_anm_modes(pdb_path: *const c_char, n_modes: usize, cutoff: f64, rmsd: f64, modes_out: *mut f64,
                        eigenvalues_out: *mut f64) -> c_int;
    pub fn ld_anm_last_kernel_ms(ms_out: *mut f64) -> c_int;
    pub fn ld_swarm_diameter2(xyz: *const i32, n: usize, d2_out: *mut u64) -> c_int;
    pub fn ld_swarm_shell(atoms: *const i32, bead: *const u8, n: usize, spacing: i32, nodes_out: *mut i32, cap: usize,
                          count_out: *mut usize, lattice_nodes_out: *mut u64) -> c_int;
    pub fn ld_swarm_centres(points: *const i32, n: usize, max_centres: usize, cover: i32, index_out: *mut u32, gap2_out: *mut u64,
                            n_out: *mut usize) -> c_int;
    pub fn ld_initial_poses(seed: u64, glowworms: usize, swarm: usize, first: usize, n: usize, centre: *const f64, radius: f64,
                            rec_points: *const f64, n_rec: usize, lig_points: *const f64, n_lig: usize, anm_rec: usize,
                            anm_lig: usize, rows_out: *mut f64, draws_out: *mut u64) -> c_int;
    pub fn ld_prepare_pdb(in_path: *const c_char, out_path: *const c_char, keep_flags: c_int, atoms_out: *mut usize,
                          centre_out: *mut f64) -> c_int;
    pub fn ld_setup_last_kernel_ms(ms_out: *mut f64) -> c_int;
    // Solvent-accessible surface (include/lightdock_hip.h, "Solvent-accessible surface"): Shrake-Rupley on integer thousandths
    pub fn ld_complex_create(receptor_pdb: *const c_char, ligand_pdb: *const c_char, rec_nmodes: *const f64, rec_nmodes_len: usize,
                             rec_num_anm: usize, lig_nmodes: *const f64, lig_nmodes_len: usize, lig_num_anm: usize) -> *mut ld_complex;
    pub fn ld_complex_destroy(c: *mut ld_complex);
    pub fn ld_complex_pose_len(c: *const ld_complex) -> usize;
    pub fn ld_complex_num_atoms(c: *const ld_complex, side: c_int) -> usize;
    pub fn ld_sasa_directions(out: *mut i32) -> c_int;
    pub fn ld_complex_sasa_radii(c: *const ld_complex, side: c_int, radii_out: *mut u32) -> c_int;
    pub fn ld_complex_sasa(c: *mut ld_complex, n: usize, poses: *const f64, stride: usize, probe: f64, sums: *mut u64,
                           free_counts: *mut u8, bound_counts: *mut u8) -> c_int;
    pub fn ld_ccs_frames(out: *mut i32) -> c_int;
    pub fn ld_complex_ccs(c: *mut ld_complex, n: usize, poses: *const f64, stride: usize, what: c_int, probe: f64, cell: f64,
                          counts: *mut u32, sums: *mut u64) -> c_int;
    pub fn ld_complex_saxs_classes(c: *const ld_complex, side: c_int, class_out: *mut u8) -> c_int;
    pub fn ld_saxs_form_factors(q: *const f64, n_q: usize, f_out: *mut f64) -> c_int;
    pub fn ld_saxs_sinc(q: *const f64, n_q: usize, width: u32, bins: usize, s_out: *mut f64) -> c_int;
    pub fn ld_complex_distance_histogram(c: *mut ld_complex, n: usize, poses: *const f64, stride: usize, width: u32, bins: usize,
                                         counts: *mut u32) -> c_int;
    pub fn ld_saxs_debye(n: usize, counts: *const u32, width: u32, bins: usize, class_atoms: *const u32, q: *const f64, n_q: usize,
                         intensity: *mut f64) -> c_int;
    pub fn ld_complex_saxs(c: *mut ld_complex, n: usize, poses: *const f64, stride: usize, width: u32, bins: usize, q: *const f64,
                           n_q: usize, intensity: *mut f64, counts: *mut u32) -> c_int;
    pub fn ld_complex_saxs_chunk(c: *mut ld_complex, poses: usize) -> c_int;
    pub fn ld_saxs_fit(n: usize, n_q: usize, intensity: *const f64, i_exp: *const f64, sigma: *const f64, scale_out: *mut f64,
                       chi2_out: *mut f64) -> c_int;
    pub fn ld_density_create(rho: *const f32, n: *const u32, origin: *const i32, step: *const u32, threshold: f64) -> *mut ld_density;
    pub fn ld_density_destroy(d: *mut ld_density);
    pub fn ld_density_info(d: *const ld_density, n_voxels: *mut u64, s_e: *mut u64, s_ee: *mut u64, scale: *mut f64) -> c_int;
    pub fn ld_density_voxels(d: *const ld_density, voxels_out: *mut u32) -> c_int;
    pub fn ld_density_kernel(sigma: u32, table_out: *mut u32, length_out: *mut u32, shift_out: *mut u32) -> c_int;
    pub fn ld_complex_density_fit(c: *mut ld_complex, d: *mut ld_density, n: usize, poses: *const f64, stride: usize, sigma: u32,
                                  out: *mut ld_density_sums) -> c_int;
    pub fn ld_complex_simulate_density(c: *mut ld_complex, d: *mut ld_density, n: usize, poses: *const f64, stride: usize, sigma: u32,
                                       grid: *mut u32) -> c_int;
    pub fn ld_density_scores(d: *const ld_density, n: usize, sums: *const ld_density_sums, cc: *mut f64, ccm: *mut f64,
                             inside: *mut f64) -> c_int;
    pub fn ld_complex_density_chunk(c: *mut ld_complex, poses: usize) -> c_int;
}

fn last_error() -> String {
    unsafe { CStr::from_ptr(ld_last_error()).to_string_lossy().into_owned() }
}

/// The vectors of a `DFIREDockingModel` / `DNADockingModel` (src/dfire.rs:104-112, src/dna.rs:235-246),
/// with `active_restraints` flattened to CSR (group order is irrelevant, src/scoring.rs:21-36).
#[derive(Default)]
pub struct ModelArrays {
    pub coordinates: Vec<[f64; 3]>,
    pub dfire_types: Vec<u32>,
    pub ele_charges: Vec<f64>,
    pub vdw_charges: Vec<f64>,
    pub vdw_radii: Vec<f64>,
    pub membrane: Vec<u32>,
    pub restraint_offsets: Vec<u32>,
    pub restraint_atoms: Vec<u32>,
    pub num_anm: usize,
    pub nmodes: Vec<f64>,
}

impl ModelArrays {
    fn view(&self) -> LdMolecule {
        let opt = |v: &Vec<f64>| if v.is_empty() { std::ptr::null() } else { v.as_ptr() };
        LdMolecule {
            n_atoms: self.coordinates.len(),
            coordinates: self.coordinates.as_ptr() as *const f64,
            dfire_types: if self.dfire_types.is_empty() { std::ptr::null() } else { self.dfire_types.as_ptr() },
            ele_charges: opt(&self.ele_charges),
            vdw_charges: opt(&self.vdw_charges),
            vdw_radii: opt(&self.vdw_radii),
            n_membrane: self.membrane.len(),
            membrane: self.membrane.as_ptr(),
            n_restraint_groups: self.restraint_offsets.len().saturating_sub(1),
            restraint_offsets: self.restraint_offsets.as_ptr(),
            restraint_atoms: self.restraint_atoms.as_ptr(),
            num_anm: self.num_anm,
            nmodes: opt(&self.nmodes),
        }
    }
}

/// Thread-compatibility: `ld_scorer_energy` reuses the handle's device workspaces and its stream, so a
/// handle serves ONE thread at a time.  The raw pointer field makes `HipScore` neither `Send` nor
/// `Sync` (which the compiler then enforces): exactly what the reference needs, whose `Score` trait has
/// no `Send + Sync` bound and whose binary scores on one worker thread (src/bin/lightdock-rust.rs:79-85).
/// A multi-threaded host creates one `HipScore` per thread (one per GPU in practice).
pub struct HipScore {
    handle: *mut c_void,
}

impl HipScore {
    /// `method`: 0 DFIRE (needs `potential`, the 169*169*20 values of data/DCparams), 1 DNA, 2 PYDOCK.
    /// Panics where the reference's constructors panic.
    pub fn new(method: i32, receptor: &ModelArrays, ligand: &ModelArrays, use_anm: bool, potential: Option<&[f64]>) -> Self {
        let desc = LdScorerDesc {
            method,
            use_anm: use_anm as c_int,
            receptor: receptor.view(),
            ligand: ligand.view(),
            potential: potential.map_or(std::ptr::null(), |p| p.as_ptr()),
        };
        unsafe {
            if ld_init(-1) != 0 {
                panic!("{}", last_error());
            }
            let handle = ld_scorer_create(&desc);
            if handle.is_null() {
                panic!("{}", last_error());
            }
            HipScore { handle }
        }
    }

    pub fn pose_len(&self) -> usize {
        unsafe { ld_scorer_pose_len(self.handle) }
    }

    /// `Score::energy` (src/scoring.rs:11-19); `rotation` = (w, x, y, z).
    pub fn energy(&self, translation: &[f64], rotation: [f64; 4], rec_nmodes: &[f64], lig_nmodes: &[f64]) -> f64 {
        let ptr = |v: &[f64]| if v.is_empty() { std::ptr::null() } else { v.as_ptr() };
        let mut e = 0.0;
        let rc = unsafe { ld_scorer_energy(self.handle, translation.as_ptr(), rotation.as_ptr(), ptr(rec_nmodes), ptr(lig_nmodes), &mut e) };
        assert_eq!(rc, 0, "{}", last_error());
        e
    }

    /// All glowworms that moved, in one launch (Swarm::update_luciferin, src/swarm.rs:66-70).
    pub fn energy_batch(&self, poses: &[f64]) -> Vec<f64> {
        let stride = self.pose_len();
        assert_eq!(poses.len() % stride, 0);
        let n = poses.len() / stride;
        let mut out = vec![0.0; n];
        let rc = unsafe { ld_scorer_energy_batch(self.handle, n, poses.as_ptr(), stride, out.as_mut_ptr()) };
        assert_eq!(rc, 0, "{}", last_error());
        out
    }
}

impl Drop for HipScore {
    fn drop(&mut self) {
        unsafe { ld_scorer_destroy(self.handle) }
    }
}

/// `GSO` (src/lib.rs:21-58) for `n_swarms` independent swarms on the device.
pub struct HipGso<'a> {
    handle: *mut c_void,
    _scorer: &'a HipScore,
}

impl<'a> HipGso<'a> {
    pub fn new(scorer: &'a HipScore, n_swarms: usize, n_glowworms: usize, positions: &[f64], seeds: Option<&[u64]>) -> Self {
        assert_eq!(positions.len(), n_swarms * n_glowworms * scorer.pose_len());
        let handle = unsafe {
            ld_gso_create(scorer.handle, n_swarms, n_glowworms, positions.as_ptr(), seeds.map_or(std::ptr::null(), |s| s.as_ptr()))
        };
        if handle.is_null() {
            panic!("{}", last_error());
        }
        HipGso { handle, _scorer: scorer }
    }

    /// GSO::run (src/lib.rs:46-58) incl. the save cadence (step 1 and every 10th).
    pub fn run(&mut self, steps: u32, output_directories: &[String]) {
        let mut done = 0u32;
        while done < steps {
            let next = if done == 0 { 1 } else { steps.min((done / 10 + 1) * 10) };
            assert_eq!(unsafe { ld_gso_run(self.handle, next - done) }, 0, "{}", last_error());
            done = next;
            if done % 10 == 0 || done == 1 {
                // one device read for all swarms, files written by threads (ld_gso_save_many); a single
                // swarm goes through ld_gso_save, the 1:1 counterpart of Swarm::save (src/swarm.rs:128-167)
                if output_directories.len() == 1 {
                    let c = CString::new(output_directories[0].as_str()).unwrap();
                    if unsafe { ld_gso_save(self.handle, 0, done, c.as_ptr()) } != 0 {
                        panic!("Error saving GSO output: {:?}", last_error());
                    }
                } else {
                    let owned: Vec<CString> = output_directories.iter().map(|d| CString::new(d.as_str()).unwrap()).collect();
                    let ptrs: Vec<*const c_char> = owned.iter().map(|c| c.as_ptr()).collect();
                    let ids: Vec<usize> = (0..owned.len()).collect();
                    if unsafe { ld_gso_save_many(self.handle, ids.len(), ids.as_ptr(), ptrs.as_ptr(), done) } != 0 {
                        panic!("Error saving GSO output: {:?}", last_error());
                    }
                }
            }
        }
    }
}

impl<'a> Drop for HipGso<'a> {
    fn drop(&mut self) {
        unsafe { ld_gso_destroy(self.handle) }
    }
}
