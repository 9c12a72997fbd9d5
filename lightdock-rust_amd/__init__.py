"""lightdock-rust_amd -- Python view of the C ABI in include/lightdock_hip.h.

This package is plumbing for tests, bench.py and the multi-GPU launcher: it loads
``lib/liblightdock_hip.so`` (hand-written HIP kernels for gfx950 + the C++ host side) with
ctypes and mirrors the reference's operator interface for the GSO + DFIRE/DNA path
(``Score::energy``, ``GSO::new/run``; lightdock-rust src/scoring.rs:11-19, src/lib.rs:27-58).

There is no CPU fallback anywhere in here: if the shared library is missing, or no
MI355X is visible when a scorer is created, the call raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "liblightdock_hip.so")
# A/B tooling (tools/ab6.sh): LIGHTDOCK_HIP_VARIANT=<name> loads lib/variants/<name>.so -- a build of the same sources with extra
# flags, tools/build_variant.sh -- instead of the installed library, so that no script has to copy a variant over it (a diagnostic
# build left installed by an interrupted script would give wrong sums silently).  A variant that does not exist is an error.
if os.environ.get("LIGHTDOCK_HIP_VARIANT"):
    LIB_PATH = os.path.join(_HERE, "lib", "variants", os.environ["LIGHTDOCK_HIP_VARIANT"] + ".so")
CLI_PATH = os.path.join(_HERE, "bin", "lightdock-hip")
INCLUDE_DIR = os.path.normpath(os.path.join(_HERE, "..", "include"))

METHOD_DFIRE = 0
METHOD_DNA = 1
METHOD_PYDOCK = 2
DFIRE_TABLE_LEN = 169 * 169 * 20
METHODS = {"dfire": METHOD_DFIRE, "dna": METHOD_DNA, "pydock": METHOD_PYDOCK}


class LightdockError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("lightdock_hip status %d: %s" % (status, message))
        self.status = status


class _KernelInfo(C.Structure):
    _fields_ = [("pair_kernel_name", C.c_char_p), ("block_threads", C.c_uint32), ("receptor_chunks", C.c_uint32),
                ("lds_bytes", C.c_uint32), ("pair_tests_per_pose", C.c_uint64), ("stream_bytes_per_pose", C.c_uint64)]


class _Molecule(C.Structure):
    _fields_ = [("n_atoms", C.c_size_t), ("coordinates", C.c_void_p), ("dfire_types", C.c_void_p),
                ("ele_charges", C.c_void_p), ("vdw_charges", C.c_void_p), ("vdw_radii", C.c_void_p),
                ("n_membrane", C.c_size_t), ("membrane", C.c_void_p), ("n_restraint_groups", C.c_size_t),
                ("restraint_offsets", C.c_void_p), ("restraint_atoms", C.c_void_p), ("num_anm", C.c_size_t),
                ("nmodes", C.c_void_p)]


class _ScorerDesc(C.Structure):
    _fields_ = [("method", C.c_int), ("use_anm", C.c_int), ("receptor", _Molecule), ("ligand", _Molecule),
                ("potential", C.c_void_p)]


class _GroupEnergies(C.Structure):
    _fields_ = [("group_of_atom", C.c_void_p), ("n_groups", C.c_size_t), ("sums", C.c_void_p), ("pairs", C.c_void_p),
                ("interface_atoms", C.c_void_p)]


class _RefineOptions(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("max_halvings", C.c_uint32), ("trans_step", C.c_double), ("rot_step", C.c_double),
                ("nm_step", C.c_double), ("slice_poses", C.c_uint32), ("reserved", C.c_uint32)]


class _RefineState(C.Structure):
    _fields_ = [("energy", C.c_void_p), ("trans_step", C.c_void_p), ("rot_cos", C.c_void_p), ("rot_sin", C.c_void_p),
                ("nm_step", C.c_void_p), ("halvings", C.c_void_p), ("accepted", C.c_void_p), ("evaluations", C.c_void_p),
                ("frozen", C.c_void_p)]


# ld_refine_stats as a structured dtype (32 bytes, no padding)
REFINE_STATS = np.dtype([("energy_before", np.float64), ("energy_after", np.float64), ("accepted", np.uint32),
                         ("halvings", np.uint32), ("evaluations", np.uint32), ("frozen", np.uint32)])
# the per-pose arrays of ld_refine_state
REFINE_STATE = (("energy", np.float64), ("trans_step", np.float64), ("rot_cos", np.float64), ("rot_sin", np.float64),
                ("nm_step", np.float64), ("halvings", np.uint32), ("accepted", np.uint32), ("evaluations", np.uint32),
                ("frozen", np.uint8))

# ld_energy_terms as a structured dtype (72 bytes, no padding)
ENERGY_TERMS = np.dtype([("pair", np.float64, (2,)), ("score", np.float64), ("rec_restraints", np.float64),
                         ("lig_restraints", np.float64), ("membrane", np.float64), ("energy", np.float64),
                         ("pairs", np.uint32), ("rec_interface", np.uint32), ("lig_interface", np.uint32),
                         ("reserved", np.uint32)])
GROUP_NONE = 0xffffffff                # LD_GROUP_NONE

_lib = None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64 and ask for
    it by the name "libamdhip64.so"; this library asks for the soname "libamdhip64.so.7".  If
    torch is imported first both resolve to torch's copy, but the other way round the process
    would end up with two runtimes (and torch then reports no GPU).  So when a torch wheel with
    a bundled runtime is installed and not loaded yet, load that copy first; without torch the
    system runtime under /opt/rocm is used, as by the lightdock-hip binary."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
        if spec is not None and spec.origin:
            bundled = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
            if os.path.exists(bundled):
                C.CDLL(bundled, mode=C.RTLD_GLOBAL)
    except (ImportError, OSError, ValueError):
        pass


def load_library():
    """dlopen the in-tree HIP library; fail loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950); "
                          "there is no CPU fallback for the pose-energy path" % LIB_PATH)
    _share_hip_runtime_with_torch()
    lib = C.CDLL(LIB_PATH)
    vp, sz, dp = C.c_void_p, C.c_size_t, C.POINTER(C.c_double)
    lib.ld_last_error.restype = C.c_char_p
    lib.ld_version.restype = C.c_char_p
    lib.ld_init.argtypes = [C.c_int]
    lib.ld_scorer_create.restype = vp
    lib.ld_scorer_create.argtypes = [C.POINTER(_ScorerDesc)]
    lib.ld_scorer_create_from_pdb.restype = vp
    lib.ld_scorer_create_from_pdb.argtypes = [C.c_int, C.c_char_p, C.c_char_p,
                                              vp, sz, vp, sz, vp, sz, sz,
                                              vp, sz, vp, sz, vp, sz, sz, C.c_int, vp]
    lib.ld_scorer_destroy.argtypes = [vp]
    lib.ld_load_dcparams.argtypes = [C.c_char_p, vp]
    lib.ld_scorer_num_atoms.restype = sz
    lib.ld_scorer_num_atoms.argtypes = [vp, C.c_int]
    lib.ld_scorer_pose_len.restype = sz
    lib.ld_scorer_pose_len.argtypes = [vp]
    lib.ld_scorer_method.argtypes = [vp]
    lib.ld_scorer_model_arrays.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    lib.ld_scorer_set_stream.argtypes = [vp, vp]
    lib.ld_scorer_energy.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.ld_scorer_energy_batch.argtypes = [vp, sz, vp, sz, vp]
    lib.ld_scorer_energy_batch_device.argtypes = [vp, sz, vp, sz, vp, vp, vp]
    lib.ld_scorer_kernel_info.argtypes = [vp, C.POINTER(_KernelInfo)]
    lib.ld_scorer_last_block_counts.argtypes = [vp, sz, vp]
    lib.ld_scorer_bm_quiet_subtiles.argtypes = [vp, vp]
    lib.ld_scorer_bm_passes.argtypes = [vp, sz, C.POINTER(sz), C.POINTER(sz)]
    lib.ld_scorer_enable_timing.argtypes = [vp, C.c_int]
    lib.ld_scorer_pair_kernel_time.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    lib.ld_gso_create.restype = vp
    lib.ld_gso_create.argtypes = [vp, sz, sz, vp, vp]
    lib.ld_gso_destroy.argtypes = [vp]
    lib.ld_gso_step.argtypes = [vp]
    lib.ld_gso_run.argtypes = [vp, C.c_uint32]
    lib.ld_gso_steps_done.restype = C.c_uint32
    lib.ld_gso_steps_done.argtypes = [vp]
    lib.ld_gso_num_evals.restype = C.c_uint64
    lib.ld_gso_num_evals.argtypes = [vp]
    lib.ld_gso_read.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp]
    lib.ld_gso_save.argtypes = [vp, sz, C.c_uint32, C.c_char_p]
    lib.ld_gso_save_many.argtypes = [vp, sz, vp, vp, C.c_uint32]
    lib.ld_cli_main.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
    lib.ld_model_from_pdb.restype = vp
    lib.ld_model_from_pdb.argtypes = [C.c_int, C.c_char_p, vp, sz, vp, sz, vp, sz, sz]
    lib.ld_model_view.argtypes = [vp, C.POINTER(_Molecule)]
    lib.ld_model_destroy.argtypes = [vp]
    lib.ld_model_num_residues.restype = sz
    lib.ld_model_num_residues.argtypes = [vp]
    lib.ld_model_residue_id.argtypes = [vp, sz, C.c_char_p, sz]
    lib.ld_model_residue_of_atom.argtypes = [vp, vp]
    lib.ld_scorer_decompose.argtypes = [vp, sz, vp, sz, vp, C.POINTER(_GroupEnergies), C.POINTER(_GroupEnergies)]
    lib.ld_scorer_decompose_info.argtypes = [vp, C.POINTER(sz), C.POINTER(C.c_double)]
    lib.ld_scorer_refine.argtypes = [vp, C.POINTER(_RefineOptions), sz, vp, sz, vp, vp, vp]
    lib.ld_scorer_refine_info.argtypes = [vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    lib.ld_refine_plan.argtypes = [sz, sz, sz, C.c_uint32, C.c_uint32, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
    lib.ld_refine_trials.argtypes = [sz, sz, vp, sz, C.POINTER(_RefineState), vp, sz, vp]
    lib.ld_refine_select.argtypes = [sz, sz, vp, sz, C.POINTER(_RefineState), vp, C.c_uint32, vp]
    lib.ld_dfire_bin_lut.argtypes = [vp, vp, C.POINTER(C.c_double)]
    lib.ld_dfire_packed_lut.argtypes = [C.c_int, C.c_double, vp, C.POINTER(C.c_double)]
    lib.ld_dfire_bm_lut.argtypes = [C.c_double, C.c_double, vp, C.POINTER(C.c_double)]
    lib.ld_stdrng_key.argtypes = [C.c_uint64, vp]
    lib.ld_spatial_tile_order.restype = sz
    lib.ld_spatial_tile_order.argtypes = [vp, sz, vp]
    lib.ld_complex_create.restype = vp
    lib.ld_complex_create.argtypes = [C.c_char_p, C.c_char_p, vp, sz, sz, vp, sz, sz]
    lib.ld_complex_destroy.argtypes = [vp]
    lib.ld_complex_pose_len.restype = sz
    lib.ld_complex_pose_len.argtypes = [vp]
    lib.ld_complex_num_atoms.restype = sz
    lib.ld_complex_num_atoms.argtypes = [vp, C.c_int]
    lib.ld_complex_coordinates.argtypes = [vp, sz, vp, sz, vp]
    lib.ld_complex_cluster.argtypes = [vp, sz, sz, vp, sz, vp, C.c_double, vp, vp, vp]
    lib.ld_complex_cluster_ranked.argtypes = [vp, sz, vp, sz, vp, C.c_double, C.c_int, vp, vp, vp]
    lib.ld_complex_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_double)]
    lib.ld_complex_write_pdb.argtypes = [vp, vp, C.c_char_p]
    lib.ld_complex_num_residues.restype = sz
    lib.ld_complex_num_residues.argtypes = [vp, C.c_int]
    lib.ld_complex_residue_id.argtypes = [vp, C.c_int, sz, C.c_char_p, sz]
    lib.ld_complex_residue_of_atom.argtypes = [vp, C.c_int, vp]
    lib.ld_complex_contacts.argtypes = [vp, sz, vp, sz, C.c_double, vp, vp]
    lib.ld_complex_pair_contacts.argtypes = [vp, sz, vp, sz, C.c_double, vp, vp, sz, C.POINTER(sz)]
    lib.ld_complex_cluster_fcc.argtypes = [vp, sz, vp, sz, vp, C.c_double, C.c_double, C.c_uint32, vp, vp, vp, vp, vp]
    lib.ld_fcc_common.argtypes = [sz, vp, vp, vp]
    lib.ld_fcc_cluster.argtypes = [sz, vp, vp, vp, C.c_double, C.c_uint32, vp, vp, vp, vp]
    lib.ld_fcc_last_kernel_ms.argtypes = [dp]
    lib.ld_sasa_directions.argtypes = [vp]
    lib.ld_complex_sasa_radii.argtypes = [vp, C.c_int, vp]
    lib.ld_complex_sasa.argtypes = [vp, sz, vp, sz, C.c_double, vp, vp, vp]
    lib.ld_ccs_frames.argtypes = [vp]
    lib.ld_complex_ccs.argtypes = [vp, sz, vp, sz, C.c_int, C.c_double, C.c_double, vp, vp]
    lib.ld_complex_crosslinks.argtypes = [vp, sz, vp, sz, sz, vp, C.c_double, C.c_double, C.c_double, C.c_double, vp, vp]
    lib.ld_complex_saxs_classes.argtypes = [vp, C.c_int, vp]
    lib.ld_saxs_form_factors.argtypes = [vp, sz, vp]
    lib.ld_saxs_sinc.argtypes = [vp, sz, C.c_uint32, sz, vp]
    lib.ld_complex_distance_histogram.argtypes = [vp, sz, vp, sz, C.c_uint32, sz, vp]
    lib.ld_saxs_debye.argtypes = [sz, vp, C.c_uint32, sz, vp, vp, sz, vp]
    lib.ld_complex_saxs.argtypes = [vp, sz, vp, sz, C.c_uint32, sz, vp, sz, vp, vp]
    lib.ld_complex_saxs_chunk.argtypes = [vp, sz]
    lib.ld_saxs_fit.argtypes = [sz, sz, vp, vp, vp, vp, vp]
    lib.ld_density_create.restype = vp
    lib.ld_density_create.argtypes = [vp, vp, vp, vp, C.c_double]
    lib.ld_density_destroy.argtypes = [vp]
    lib.ld_density_info.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), dp]
    lib.ld_density_voxels.argtypes = [vp, vp]
    lib.ld_density_kernel.argtypes = [C.c_uint32, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.ld_complex_density_fit.argtypes = [vp, vp, sz, vp, sz, C.c_uint32, vp]
    lib.ld_complex_simulate_density.argtypes = [vp, vp, sz, vp, sz, C.c_uint32, vp]
    lib.ld_density_scores.argtypes = [vp, sz, vp, vp, vp, vp]
    lib.ld_complex_density_chunk.argtypes = [vp, sz]
    lib.ld_complex_set_reference.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_double, C.c_double]
    lib.ld_complex_reference_counts.argtypes = [vp, vp]
    lib.ld_complex_native_pairs.argtypes = [vp, vp]
    lib.ld_complex_assess.argtypes = [vp, sz, vp, sz, vp, vp, vp]
    lib.ld_anm_nodes.argtypes = [C.c_char_p, vp, C.POINTER(sz)]
    lib.ld_anm_modes_xyz.argtypes = [vp, sz, sz, C.c_double, vp, vp]
    lib.ld_anm_modes.argtypes = [C.c_char_p, sz, C.c_double, C.c_double, vp, vp]
    lib.ld_anm_last_kernel_ms.argtypes = [dp]
    lib.ld_swarm_diameter2.argtypes = [vp, sz, C.POINTER(C.c_uint64)]
    lib.ld_swarm_shell.argtypes = [vp, vp, sz, C.c_int32, vp, sz, C.POINTER(sz), C.POINTER(C.c_uint64)]
    lib.ld_swarm_centres.argtypes = [vp, sz, sz, C.c_int32, vp, vp, C.POINTER(sz)]
    lib.ld_initial_poses.argtypes = [C.c_uint64, sz, sz, sz, sz, vp, C.c_double, vp, sz, vp, sz, sz, sz, vp, vp]
    lib.ld_prepare_pdb.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(sz), vp]
    lib.ld_setup_last_kernel_ms.argtypes = [dp]
    _lib = lib
    return lib


def _check(status):
    if status != 0:
        raise LightdockError(status, load_library().ld_last_error().decode())


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _strings(items):
    items = [s.encode() for s in (items or [])]
    arr = (C.c_char_p * max(1, len(items)))(*items)
    return C.cast(arr, C.c_void_p), len(items), arr


def init(device=-1):
    _check(load_library().ld_init(device))


def device_count():
    return load_library().ld_device_count()


def load_dcparams(path):
    out = np.empty(DFIRE_TABLE_LEN, dtype=np.float64)
    _check(load_library().ld_load_dcparams(os.fsencode(path), _ptr(out)))
    return out


def _np_from(ptr, n, ctype, dtype):
    if not ptr or n == 0:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(n,)).copy()


def model_from_pdb(method, pdb_path, active=(), passive=(), nmodes=None, num_anm=0):
    """Host-side DockingModel::new (src/dfire.rs:115-190, src/dna.rs:249-364); no GPU involved.
    Returns the ld_molecule fields as a dict of numpy arrays (usable with Scorer.from_arrays), and the model's residues:
    "residues", the ids ("A.SER.467") of the runs of consecutive atoms with one id, and "residue_of_atom", a group map
    for Scorer.decompose."""
    lib = load_library()
    method = METHODS.get(method, method)
    a, na, k1 = _strings(active)
    p, npas, k2 = _strings(passive)
    nm = None if nmodes is None else _f64(nmodes).ravel()
    h = lib.ld_model_from_pdb(method, os.fsencode(pdb_path), a, na, p, npas, _ptr(nm), 0 if nm is None else nm.size, num_anm)
    if not h:
        raise LightdockError(-1, lib.ld_last_error().decode())
    h = C.c_void_p(h)
    try:
        v = _Molecule()
        _check(lib.ld_model_view(h, C.byref(v)))
        n = v.n_atoms
        out = {"coordinates": _np_from(v.coordinates, 3 * n, C.c_double, np.float64).reshape(n, 3),
               "membrane": _np_from(v.membrane, v.n_membrane, C.c_uint32, np.uint32), "num_anm": int(v.num_anm)}
        offs = _np_from(v.restraint_offsets, v.n_restraint_groups + 1, C.c_uint32, np.uint32)
        out["restraint_offsets"] = offs
        out["restraint_atoms"] = _np_from(v.restraint_atoms, int(offs[-1]) if len(offs) else 0, C.c_uint32, np.uint32)
        if v.dfire_types:
            out["dfire_types"] = _np_from(v.dfire_types, n, C.c_uint32, np.uint32)
        for k in ("ele_charges", "vdw_charges", "vdw_radii"):
            if getattr(v, k):
                out[k] = _np_from(getattr(v, k), n, C.c_double, np.float64)
        if v.nmodes:
            out["nmodes"] = _np_from(v.nmodes, int(v.num_anm) * n * 3, C.c_double, np.float64)
        buf = C.create_string_buffer(64)
        out["residues"] = []
        for i in range(lib.ld_model_num_residues(h)):
            _check(lib.ld_model_residue_id(h, i, buf, len(buf)))
            out["residues"].append(buf.value.decode())
        out["residue_of_atom"] = np.zeros(n, dtype=np.uint32)
        _check(lib.ld_model_residue_of_atom(h, _ptr(out["residue_of_atom"])))
        return out
    finally:
        lib.ld_model_destroy(h)


def dfire_bin_lut():
    lut = np.zeros(901, dtype=np.uint8)
    steps = np.zeros(21, dtype=np.float64)
    d2 = C.c_double()
    _check(load_library().ld_dfire_bin_lut(_ptr(lut), _ptr(steps), C.byref(d2)))
    return lut, steps, d2.value


def dfire_packed_lut(cells_per_unit=2, ubound=256.0):
    """(words, eps) of the default DFIRE kernel's cell LUT, see ld_dfire_packed_lut in the header."""
    words = np.zeros(1028 * cells_per_unit, dtype=np.uint32)
    eps = C.c_double()
    _check(load_library().ld_dfire_packed_lut(cells_per_unit, ubound, _ptr(words), C.byref(eps)))
    return words, eps.value


def dfire_bm_lut(ubound=1024.0, lig_extent=45.0):
    """(codes, eps in LUT cells) of the block-major DFIRE kernel's cell LUT, see ld_dfire_bm_lut in the header."""
    codes = np.zeros(14592, dtype=np.uint8)
    eps = C.c_double()
    _check(load_library().ld_dfire_bm_lut(C.c_double(ubound), C.c_double(lig_extent), _ptr(codes), C.byref(eps)))
    return codes, eps.value


def dfire_route_frames(rec_xyz, lig_xyz, anm=False, rec_types=None):
    """The record frames of the two culled DFIRE routes for a complex's coordinates, see ld_dfire_route_frames in the header:
    {"bm": dict(centre, ubound, lig_extent, eps, takes, sub_axis, sub_diag), "packed": dict(centre, kappa, ubound, eps, cells,
    takes)}.  rec_types: the receptor's DFIRE types (its subtiles then enter the block-major bound, as in the scorer)."""
    rec, lig = _f64(rec_xyz).reshape(-1, 3), _f64(lig_xyz).reshape(-1, 3)
    types = None if rec_types is None else np.ascontiguousarray(rec_types, dtype=np.uint32)
    if types is not None and types.shape != (rec.shape[0],):
        raise ValueError("one DFIRE type per receptor atom")
    bm, packed = np.zeros(9), np.zeros(8)
    lib = load_library()
    lib.ld_dfire_route_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    _check(lib.ld_dfire_route_frames(_ptr(rec), _ptr(types), rec.shape[0], _ptr(lig), lig.shape[0], 1 if anm else 0, _ptr(bm), _ptr(packed)))
    return {"bm": dict(centre=bm[:3].copy(), ubound=bm[3], lig_extent=bm[4], eps=bm[5], takes=bool(bm[6]), sub_axis=bm[7], sub_diag=bm[8]),
            "packed": dict(centre=packed[:3].copy(), kappa=packed[3], ubound=packed[4], eps=packed[5], cells=int(packed[6]),
                           takes=bool(packed[7]))}


def dfire_bm_fix_scale(rec_xyz, reach, table_vmax):
    """(reach count, extra bits, scale) of the block-major kernel's fixed-point sums, see ld_dfire_bm_fix_scale in the header."""
    xyz = _f64(rec_xyz).reshape(-1, 3)
    count, extra, scale = C.c_uint64(), C.c_int(), C.c_double()
    lib = load_library()
    lib.ld_dfire_bm_fix_scale.argtypes = [C.c_void_p, C.c_size_t, C.c_double, C.c_double, C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_double)]
    _check(lib.ld_dfire_bm_fix_scale(_ptr(xyz), xyz.shape[0], C.c_double(reach), C.c_double(table_vmax), C.byref(count), C.byref(extra), C.byref(scale)))
    return count.value, extra.value, scale.value


BM_WS_REGIONS = 22


def dfire_bm_workspace(n_rt, n_lt, cap, sets, waves, anm=False, counts=False, debug=False):
    """The block-major kernels' workspace for one batch shape, see ld_dfire_bm_workspace in the header:
    {region: dict(buffer=name, buffer_bytes=, base=, stride=, bytes=)}."""
    names = (C.c_char_p * (2 * BM_WS_REGIONS))()
    rows = np.zeros((BM_WS_REGIONS, 5), dtype=np.uint64)
    flags = (1 if anm else 0) | (2 if counts else 0) | (4 if debug else 0)
    lib = load_library()
    lib.ld_dfire_bm_workspace.argtypes = [C.c_size_t] * 5 + [C.c_int, C.c_void_p, C.c_void_p]   # (bound here: a library variant of an older build loads without it)
    _check(lib.ld_dfire_bm_workspace(n_rt, n_lt, cap, sets, waves, flags, C.cast(names, C.c_void_p), _ptr(rows)))
    return {names[2 * r].decode(): dict(buffer=names[2 * r + 1].decode(), buffer_bytes=int(rows[r, 1]), base=int(rows[r, 2]),
                                        stride=int(rows[r, 3]), bytes=int(rows[r, 4])) for r in range(BM_WS_REGIONS)}


def spatial_tile_order(xyz):
    """Tile order of the DFIRE kernel: slot -> atom index (UINT32_MAX = padding)."""
    xyz = _f64(xyz).reshape(-1, 3)
    n = xyz.shape[0]
    out = np.zeros((n + 63) // 64 * 64, dtype=np.uint32)
    got = load_library().ld_spatial_tile_order(_ptr(xyz), n, _ptr(out))
    if got != out.size:
        raise LightdockError(-1, load_library().ld_last_error().decode())
    return out


def dfire_tile_layout(xyz, dfire_types):
    """(order, type_perm) the DFIRE scorer uses for one molecule: order[slot] = atom index
    (UINT32_MAX = padding), type_perm[type] = number in the patch layout of the potential."""
    xyz = _f64(xyz).reshape(-1, 3)
    types = np.ascontiguousarray(dfire_types, dtype=np.uint32)
    n = xyz.shape[0]
    order = np.zeros((n + 63) // 64 * 64, dtype=np.uint32)
    perm = np.zeros(169, dtype=np.uint32)
    lib = load_library()
    lib.ld_dfire_tile_layout.restype = C.c_size_t
    lib.ld_dfire_tile_layout.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    got = lib.ld_dfire_tile_layout(_ptr(xyz), _ptr(types), n, _ptr(order), _ptr(perm))
    if got != order.size:
        raise LightdockError(-1, lib.ld_last_error().decode())
    return order, perm


def stdrng_key(seed):
    key = np.zeros(8, dtype=np.uint32)
    load_library().ld_stdrng_key(seed, _ptr(key))
    return key


class Scorer:
    """A `Box<dyn Score>`: DFIRE::new / DNA::new (src/dfire.rs:201-234, src/dna.rs:375-408)."""

    def __init__(self, handle, keep=()):
        if not handle:
            raise LightdockError(-1, load_library().ld_last_error().decode())
        self._h = C.c_void_p(handle)
        self._keep = keep
        self.lib = load_library()

    @classmethod
    def from_pdb(cls, method, receptor_pdb, ligand_pdb, rec_active=(), rec_passive=(), rec_nmodes=None, rec_num_anm=0,
                 lig_active=(), lig_passive=(), lig_nmodes=None, lig_num_anm=0, use_anm=False, potential=None):
        lib = load_library()
        method = METHODS.get(method, method)
        ra, nra, k1 = _strings(rec_active)
        rp, nrp, k2 = _strings(rec_passive)
        la, nla, k3 = _strings(lig_active)
        lp, nlp, k4 = _strings(lig_passive)
        rnm = None if rec_nmodes is None else _f64(rec_nmodes).ravel()
        lnm = None if lig_nmodes is None else _f64(lig_nmodes).ravel()
        pot = None if potential is None else _f64(potential)
        if pot is not None and pot.size != DFIRE_TABLE_LEN:
            raise ValueError("DFIRE potential must have %d values" % DFIRE_TABLE_LEN)
        h = lib.ld_scorer_create_from_pdb(method, os.fsencode(receptor_pdb), os.fsencode(ligand_pdb),
                                          ra, nra, rp, nrp, _ptr(rnm), 0 if rnm is None else rnm.size, rec_num_anm,
                                          la, nla, lp, nlp, _ptr(lnm), 0 if lnm is None else lnm.size, lig_num_anm,
                                          1 if use_anm else 0, _ptr(pot))
        return cls(h, keep=(k1, k2, k3, k4))

    @classmethod
    def from_arrays(cls, method, receptor, ligand, use_anm=False, potential=None):
        """receptor / ligand: dicts with the fields of ld_molecule (numpy arrays)."""
        lib = load_library()
        method = METHODS.get(method, method)
        keep = []

        def mol(d):
            m = _Molecule()
            coords = _f64(d["coordinates"]).reshape(-1, 3)
            keep.append(coords)
            m.n_atoms = coords.shape[0]
            m.coordinates = _ptr(coords)
            for name, dt in (("dfire_types", np.uint32), ("ele_charges", np.float64), ("vdw_charges", np.float64),
                             ("vdw_radii", np.float64), ("membrane", np.uint32), ("restraint_offsets", np.uint32),
                             ("restraint_atoms", np.uint32), ("nmodes", np.float64)):
                v = d.get(name)
                if v is not None:
                    v = np.ascontiguousarray(v, dtype=dt).ravel()
                    keep.append(v)
                    setattr(m, name, _ptr(v))
            m.n_membrane = 0 if d.get("membrane") is None else len(d["membrane"])
            offs = d.get("restraint_offsets")
            m.n_restraint_groups = 0 if offs is None else len(offs) - 1
            m.num_anm = int(d.get("num_anm", 0))
            return m

        desc = _ScorerDesc()
        desc.method = method
        desc.use_anm = 1 if use_anm else 0
        desc.receptor = mol(receptor)
        desc.ligand = mol(ligand)
        if potential is not None:
            pot = _f64(potential)
            keep.append(pot)
            desc.potential = _ptr(pot)
        return cls(lib.ld_scorer_create(C.byref(desc)), keep=tuple(keep))

    def close(self):
        if self._h:
            self.lib.ld_scorer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    @property
    def pose_len(self):
        return self.lib.ld_scorer_pose_len(self._h)

    def num_atoms(self, side):
        return self.lib.ld_scorer_num_atoms(self._h, side)

    def model_arrays(self, side):
        n = self.num_atoms(side)
        out = {"coordinates": np.zeros((n, 3))}
        if self.lib.ld_scorer_method(self._h) == METHOD_DFIRE:
            out["dfire_types"] = np.zeros(n, dtype=np.uint32)
            _check(self.lib.ld_scorer_model_arrays(self._h, side, _ptr(out["coordinates"]), _ptr(out["dfire_types"]),
                                                   None, None, None))
        else:
            for k in ("ele_charges", "vdw_charges", "vdw_radii"):
                out[k] = np.zeros(n)
            _check(self.lib.ld_scorer_model_arrays(self._h, side, _ptr(out["coordinates"]), None,
                                                   _ptr(out["ele_charges"]), _ptr(out["vdw_charges"]), _ptr(out["vdw_radii"])))
        return out

    def set_stream(self, hip_stream):
        _check(self.lib.ld_scorer_set_stream(self._h, C.c_void_p(hip_stream)))

    def energy(self, translation, rotation, rec_nmodes=None, lig_nmodes=None):
        """Score::energy (src/scoring.rs:11-19); rotation = (w, x, y, z)."""
        t, q = _f64(translation), _f64(rotation)
        rn = None if rec_nmodes is None or len(rec_nmodes) == 0 else _f64(rec_nmodes)
        ln = None if lig_nmodes is None or len(lig_nmodes) == 0 else _f64(lig_nmodes)
        out = C.c_double()
        _check(self.lib.ld_scorer_energy(self._h, _ptr(t), _ptr(q), _ptr(rn), _ptr(ln), C.byref(out)))
        return out.value

    def energy_batch(self, poses):
        poses = _f64(poses)
        if poses.ndim != 2:
            raise ValueError("poses must be (n, pose_len)")
        out = np.empty(poses.shape[0], dtype=np.float64)
        _check(self.lib.ld_scorer_energy_batch(self._h, poses.shape[0], _ptr(poses), poses.shape[1], _ptr(out)))
        return out

    def energy_batch_device(self, n, d_poses, stride, d_energies, d_active=None, d_pair_counts=None):
        """Raw device pointers (ints), asynchronous on the scorer's stream."""
        _check(self.lib.ld_scorer_energy_batch_device(self._h, n, C.c_void_p(d_poses), stride,
                                                      C.c_void_p(d_active) if d_active else None, C.c_void_p(d_energies),
                                                      C.c_void_p(d_pair_counts) if d_pair_counts else None))

    def decompose(self, poses, rec_groups=None, lig_groups=None, atoms=False):
        """Which terms make up each pose's energy and which groups of atoms carry it (ld_scorer_decompose; the definition
        is in lightdock_hip.h, "Energy decomposition").  poses: (n, >= pose_len).  rec_groups / lig_groups: a group id per
        atom of that side (GROUP_NONE: no group), e.g. model_from_pdb(...)["residue_of_atom"]; atoms=True: every atom its
        own group on the sides without a map.  Returns {"terms": structured array (n,) of ENERGY_TERMS, "rec", "lig":
        {"sums" (n, groups, 2), "pairs" (n, groups), "interface" (n, groups)} or None}.  Sums are raw, not in score units."""
        poses = _f64(poses)
        if poses.ndim != 2:
            raise ValueError("poses must be (n, pose_len)")
        n = poses.shape[0]
        out = {"terms": np.zeros(n, dtype=ENERGY_TERMS), "rec": None, "lig": None}
        structs, keep = [None, None], []
        for side, (key, groups) in enumerate((("rec", rec_groups), ("lig", lig_groups))):
            if groups is None and not atoms:
                continue
            g = _GroupEnergies()
            if groups is None:
                n_groups = self.num_atoms(side)
            else:
                gmap = np.ascontiguousarray(groups, dtype=np.uint32).ravel()
                if gmap.size != self.num_atoms(side):
                    raise ValueError("one group id per atom")
                keep.append(gmap)
                g.group_of_atom = _ptr(gmap)
                ids = gmap[gmap != GROUP_NONE]
                n_groups = int(ids.max()) + 1 if ids.size else 1
            g.n_groups = n_groups
            res = {"sums": np.zeros((n, n_groups, 2)), "pairs": np.zeros((n, n_groups), dtype=np.uint32),
                   "interface": np.zeros((n, n_groups), dtype=np.uint32)}
            g.sums, g.pairs, g.interface_atoms = _ptr(res["sums"]), _ptr(res["pairs"]), _ptr(res["interface"])
            out[key] = res
            structs[side] = g
        _check(self.lib.ld_scorer_decompose(self._h, n, _ptr(poses), poses.shape[1], _ptr(out["terms"]),
                                            None if structs[0] is None else C.byref(structs[0]),
                                            None if structs[1] is None else C.byref(structs[1])))
        return out

    def decompose_info(self):
        """{"slice": poses per pass of decompose(), "last_kernel_ms": its kernels in the last call (HIP events)}."""
        slice_poses, ms = C.c_size_t(), C.c_double()
        _check(self.lib.ld_scorer_decompose_info(self._h, C.byref(slice_poses), C.byref(ms)))
        return {"slice": slice_poses.value, "last_kernel_ms": ms.value}

    def refine(self, poses, iterations=20, trans_step=1.0, rot_step=0.1, nm_step=0.5, max_halvings=4, slice_poses=0,
               history=False):
        """Walk every pose uphill under this scorer's energy by the compass search of lightdock_hip.h, "Local refinement"
        (ld_scorer_refine).  poses: (n, >= pose_len).  Returns {"poses": (n, pose_len), "stats": structured array (n,) of
        REFINE_STATS, "history": (n, iterations) int16 or None}."""
        poses = _f64(poses)
        if poses.ndim != 2:
            raise ValueError("poses must be (n, pose_len)")
        n = poses.shape[0]
        opts = _RefineOptions(int(iterations), int(max_halvings), float(trans_step), float(rot_step), float(nm_step),
                              int(slice_poses), 0)
        out = {"poses": np.zeros((n, self.pose_len)), "stats": np.zeros(n, dtype=REFINE_STATS),
               "history": np.zeros((n, max(int(iterations), 0)), dtype=np.int16) if history else None}
        _check(self.lib.ld_scorer_refine(self._h, C.byref(opts), n, _ptr(poses), poses.shape[1], _ptr(out["poses"]),
                                         _ptr(out["stats"]), _ptr(out["history"])))
        return out

    def refine_info(self):
        """{"trials": K of this scorer, "slice": poses per pass of the last refine() (before any: the default),
        "last_kernel_ms": its device work (HIP events), "evaluations": its energy evaluations over all poses}."""
        trials, slice_poses, ms, evals = C.c_size_t(), C.c_size_t(), C.c_double(), C.c_uint64()
        _check(self.lib.ld_scorer_refine_info(self._h, C.byref(trials), C.byref(slice_poses), C.byref(ms), C.byref(evals)))
        return {"trials": trials.value, "slice": slice_poses.value, "last_kernel_ms": ms.value, "evaluations": evals.value}

    def enable_timing(self, on=True):
        _check(self.lib.ld_scorer_enable_timing(self._h, 1 if on else 0))

    def pair_kernel_time(self):
        """(total ms, launches) of the pair kernel since the last call; HIP events on the scorer's stream."""
        ms, n = C.c_double(), C.c_uint64()
        _check(self.lib.ld_scorer_pair_kernel_time(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def last_block_counts(self, n):
        """8x8 atom-pair blocks evaluated per pose in the last counting launch (culled DFIRE kernels)."""
        out = np.zeros(n, dtype=np.uint32)
        _check(self.lib.ld_scorer_last_block_counts(self._h, n, _ptr(out)))
        return out

    def bm_quiet_subtiles(self):
        """Receptor subtiles whose atoms' rows of the potential are zero against every ligand type (block-major DFIRE path)."""
        n = C.c_uint32()
        _check(self.lib.ld_scorer_bm_quiet_subtiles(self._h, C.byref(n)))
        return n.value

    def bm_passes(self, n):
        """(poses per pass, workspace sets) of a batch of n poses on the block-major DFIRE path; (0, 0) on another route."""
        pass_poses, sets = C.c_size_t(), C.c_size_t()
        _check(self.lib.ld_scorer_bm_passes(self._h, n, C.byref(pass_poses), C.byref(sets)))
        return pass_poses.value, sets.value

    def kernel_info(self):
        info = _KernelInfo()
        _check(self.lib.ld_scorer_kernel_info(self._h, C.byref(info)))
        return {"pair_kernel_name": info.pair_kernel_name.decode(), "block_threads": info.block_threads,
                "receptor_chunks": info.receptor_chunks, "lds_bytes": info.lds_bytes,
                "pair_tests_per_pose": info.pair_tests_per_pose, "stream_bytes_per_pose": info.stream_bytes_per_pose}


class GSO:
    """GSO::new / GSO::run (src/lib.rs:27-58) for a batch of independent swarms."""

    def __init__(self, scorer, positions, seeds=None):
        positions = _f64(positions)
        if positions.ndim == 2:
            positions = positions[None]
        if positions.ndim != 3 or positions.shape[2] != scorer.pose_len:
            raise ValueError("positions must be (swarms, glowworms, %d)" % scorer.pose_len)
        self.scorer = scorer
        self.lib = scorer.lib
        self.n_swarms, self.n_glowworms, self.pose_len = positions.shape
        sd = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint64)
        if sd is not None and sd.size != self.n_swarms:
            raise ValueError("one seed per swarm")
        h = self.lib.ld_gso_create(scorer.handle, self.n_swarms, self.n_glowworms, _ptr(positions), _ptr(sd))
        if not h:
            raise LightdockError(-1, self.lib.ld_last_error().decode())
        self._h = C.c_void_p(h)

    def close(self):
        if self._h:
            self.lib.ld_gso_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def step(self):
        _check(self.lib.ld_gso_step(self._h))

    def run(self, steps):
        _check(self.lib.ld_gso_run(self._h, steps))

    @property
    def steps_done(self):
        return self.lib.ld_gso_steps_done(self._h)

    @property
    def num_evals(self):
        return self.lib.ld_gso_num_evals(self._h)

    def read(self, swarm=0):
        n = self.n_glowworms
        st = {"poses": np.empty((n, self.pose_len)), "luciferin": np.empty(n), "vision_range": np.empty(n),
              "scoring": np.empty(n), "n_neighbors": np.empty(n, dtype=np.int32), "moved": np.empty(n, dtype=np.int32),
              "target": np.empty(n, dtype=np.int32)}
        _check(self.lib.ld_gso_read(self._h, swarm, _ptr(st["poses"]), _ptr(st["luciferin"]), _ptr(st["vision_range"]),
                                    _ptr(st["scoring"]), _ptr(st["n_neighbors"]), _ptr(st["moved"]), _ptr(st["target"])))
        return st

    def save(self, swarm, step, directory):
        _check(self.lib.ld_gso_save(self._h, swarm, step, os.fsencode(directory)))

    def save_many(self, swarms, step, directories):
        """gso_<step>.out of many swarms in one call (one device read, files written by threads)."""
        n = len(swarms)
        ids = (C.c_size_t * n)(*[int(s) for s in swarms])
        dirs = (C.c_char_p * n)(*[os.fsencode(d) for d in directories])
        _check(self.lib.ld_gso_save_many(self._h, n, ids, dirs, step))


SAXS_CLASSES, SAXS_PAIR_CLASSES, SAXS_MAX_BINS = 6, 21, 1024


def saxs_width(width):
    """A bin width in A -> whole thousandths; the library checks the range."""
    w = int(round(1000.0 * float(width)))
    if not 0 <= w < 2 ** 32:
        raise ValueError("width must be 0.1 .. 2.0 A")
    return w


DENSITY_SUMS = np.dtype([("s", np.uint64), ("ss", np.uint64), ("se", np.uint64), ("inside_sum", np.uint64), ("outside", np.uint32),
                         ("reserved", np.uint32)])      # ld_density_sums


def _thousandths3(v, what):
    a = np.asarray(v)
    if a.shape != (3,) or not np.all(np.isfinite(np.asarray(a, dtype=np.float64))) or np.any(a != np.rint(a)) or np.any(np.abs(np.asarray(a, dtype=np.float64)) > 2 ** 31 - 1):
        raise ValueError("%s must be three whole thousandths of an A" % what)
    return [int(x) for x in a]


class Density:
    """A density map as the fit reads it (ld_density_*; lightdock_hip.h, "Density fit"): rho (nz, ny, nx) floats, x fastest;
    origin and step in whole thousandths of an A, the centre of voxel (i, j, k) at origin + (i hx, j hy, k hz) in the run's
    frame.  Values below threshold become 0, the rest are quantised to 0 .. 32767."""

    def __init__(self, rho, origin, step, threshold=0.0):
        self.lib = load_library()
        rho = np.ascontiguousarray(rho, dtype=np.float32)
        if rho.ndim != 3:
            raise ValueError("rho must be (nz, ny, nx)")
        origin, step = _thousandths3(origin, "origin"), _thousandths3(step, "step")
        if min(step) < 0:
            raise ValueError("step must be positive")
        self.shape = rho.shape
        self.origin, self.step = tuple(origin), tuple(step)
        n = (C.c_uint32 * 3)(rho.shape[2], rho.shape[1], rho.shape[0])
        h = self.lib.ld_density_create(_ptr(rho), n, (C.c_int32 * 3)(*origin), (C.c_uint32 * 3)(*step), float(threshold))
        if not h:
            raise LightdockError(-1, self.lib.ld_last_error().decode())
        self._h = C.c_void_p(h)

    def __del__(self):
        if getattr(self, "_h", None):
            self.lib.ld_density_destroy(self._h)

    def info(self):
        """{"n": voxels, "s_e": sum E, "s_ee": sum E^2, "scale": 32767 / max rho'} (ld_density_info)."""
        n, se, see, scale = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double()
        _check(self.lib.ld_density_info(self._h, C.byref(n), C.byref(se), C.byref(see), C.byref(scale)))
        return {"n": n.value, "s_e": se.value, "s_ee": see.value, "scale": scale.value}

    def voxels(self):
        """(nz, ny, nx) uint32: the quantised voxels E (ld_density_voxels)."""
        out = np.zeros(self.shape, dtype=np.uint32)
        _check(self.lib.ld_density_voxels(self._h, _ptr(out)))
        return out


def density_kernel(sigma):
    """sigma in whole thousandths of an A -> (table (T,) uint32, shift): an atom at squared distance d2 adds
    weight * table[d2 >> shift] when d2 < T << shift (ld_density_kernel; made on the host with libm)."""
    lib = load_library()
    length, shift = C.c_uint32(), C.c_uint32()
    _check(lib.ld_density_kernel(int(sigma), None, C.byref(length), C.byref(shift)))
    table = np.zeros(length.value, dtype=np.uint32)
    _check(lib.ld_density_kernel(int(sigma), _ptr(table), C.byref(length), C.byref(shift)))
    return table, shift.value


def density_scores(density, sums):
    """sums: density_fit()'s dict, or a DENSITY_SUMS array -> (cc, ccm, inside), each (n,) (ld_density_scores; host only)."""
    if isinstance(sums, dict):
        rows = np.zeros(len(sums["s"]), dtype=DENSITY_SUMS)
        for k in ("s", "ss", "se", "inside_sum", "outside"):
            rows[k] = sums[k]
    else:
        rows = np.ascontiguousarray(sums, dtype=DENSITY_SUMS)
    n = rows.shape[0]
    cc, ccm, inside = np.zeros(n), np.zeros(n), np.zeros(n)
    _check(load_library().ld_density_scores(density._h, n, _ptr(rows), _ptr(cc), _ptr(ccm), _ptr(inside)))
    return cc, ccm, inside


class Complex:
    """LightDock's analysis of a run (ld_complex_*): posed coordinates, BSAS clustering of whole swarms and of one ranked
    list across swarms, top-model PDBs, per-pose interface contacts and residue-pair sets, clustering by common contacts, solvent-accessible
    and buried surface, SAXS profiles, the fit to a density map."""

    def __init__(self, receptor_pdb, ligand_pdb, rec_nmodes=None, rec_num_anm=0, lig_nmodes=None, lig_num_anm=0):
        self.lib = load_library()
        rnm = np.zeros(0) if rec_nmodes is None else _f64(rec_nmodes).ravel()
        lnm = np.zeros(0) if lig_nmodes is None else _f64(lig_nmodes).ravel()
        h = self.lib.ld_complex_create(os.fsencode(receptor_pdb), os.fsencode(ligand_pdb), _ptr(rnm), rnm.size, rec_num_anm,
                                       _ptr(lnm), lnm.size, lig_num_anm)
        if not h:
            raise LightdockError(-1, self.lib.ld_last_error().decode())
        self._h = C.c_void_p(h)
        self.pose_len = self.lib.ld_complex_pose_len(self._h)

    def __del__(self):
        if getattr(self, "_h", None):
            self.lib.ld_complex_destroy(self._h)

    def num_atoms(self, side):
        """0: receptor, 1: ligand, 2: the complex's CA / P atoms."""
        return self.lib.ld_complex_num_atoms(self._h, side)

    def coordinates(self, poses):
        """(n, >= pose_len) poses -> (n, receptor + ligand atoms, 3)."""
        poses = _f64(poses)
        out = np.empty((poses.shape[0], self.num_atoms(0) + self.num_atoms(1), 3))
        _check(self.lib.ld_complex_coordinates(self._h, poses.shape[0], _ptr(poses), poses.shape[1], _ptr(out)))
        return out

    def cluster(self, poses, scoring, cutoff=4.0):
        """poses (swarms, glowworms, >= pose_len), scoring (swarms, glowworms) -> dict of cluster_of, representatives
        (-1 after the last) and n_clusters."""
        poses, scoring = _f64(poses), _f64(scoring)
        if poses.ndim != 3 or scoring.shape != poses.shape[:2]:
            raise ValueError("poses must be (swarms, glowworms, pose_len), scoring (swarms, glowworms)")
        ns, ng = scoring.shape
        out = {"cluster_of": np.empty((ns, ng), dtype=np.int32), "representatives": np.empty((ns, ng), dtype=np.int32),
               "n_clusters": np.empty(ns, dtype=np.uint32)}
        _check(self.lib.ld_complex_cluster(self._h, ns, ng, _ptr(poses), poses.shape[2], _ptr(scoring), C.c_double(cutoff),
                                           _ptr(out["cluster_of"]), _ptr(out["representatives"]), _ptr(out["n_clusters"])))
        return out

    def cluster_ranked(self, poses, scoring, cutoff=4.0, atoms="complex"):
        """One ranked list of poses of any swarms, up to about a million: poses (n, >= pose_len), scoring (n,) -> a dict
        shaped like cluster()'s with ONE row: cluster_of (1, n) in input order, representatives (1, n) input indices in
        creation order (-1 after the last), n_clusters (1,).  atoms: "complex", the CA / P atoms of the whole complex
        (cluster()'s measure), or "ligand", the ligand's only (ld_complex_cluster_ranked)."""
        poses, scoring = _f64(poses), _f64(scoring)
        if poses.ndim != 2 or scoring.shape != poses.shape[:1]:
            raise ValueError("poses must be (n, pose_len), scoring (n,)")
        if atoms not in ("complex", "ligand"):
            raise ValueError('atoms must be "complex" or "ligand"')
        n = scoring.shape[0]
        out = {"cluster_of": np.empty((1, n), dtype=np.int32), "representatives": np.empty((1, n), dtype=np.int32),
               "n_clusters": np.empty(1, dtype=np.uint32)}
        _check(self.lib.ld_complex_cluster_ranked(self._h, n, _ptr(poses), poses.shape[1], _ptr(scoring), C.c_double(cutoff),
                                                  int(atoms == "ligand"), _ptr(out["cluster_of"]), _ptr(out["representatives"]),
                                                  _ptr(out["n_clusters"])))
        return out

    def last_kernel_ms(self):
        ms = C.c_double()
        _check(self.lib.ld_complex_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def num_residues(self, side):
        """0: receptor, 1: ligand."""
        return self.lib.ld_complex_num_residues(self._h, side)

    def residues(self, side):
        """Residue ids ("A.SER.467", "H.ASP.52A") of one side, in file order: the columns of contacts()."""
        buf = C.create_string_buffer(64)
        ids = []
        for i in range(self.num_residues(side)):
            _check(self.lib.ld_complex_residue_id(self._h, side, i, buf, len(buf)))
            ids.append(buf.value.decode())
        if not ids:   # a side other than 0 / 1
            _check(self.lib.ld_complex_residue_id(self._h, side, 0, buf, len(buf)))
        return ids

    def residue_of_atom(self, side):
        out = np.empty(self.num_atoms(side) if side in (0, 1) else 0, dtype=np.uint32)
        _check(self.lib.ld_complex_residue_of_atom(self._h, side, _ptr(out)))
        return out

    def contacts(self, poses, cutoff=5.0, packed=False):
        """(n, >= pose_len) poses -> {"rec": bool (n, receptor residues), "lig": bool (n, ligand residues)}: the residues
        with an atom within `cutoff` of the other molecule, on the coordinates "%8.3f" prints (ld_complex_contacts).
        packed=True: the call's uint32 words instead (bit k of word w is residue 32 w + k)."""
        poses = _f64(poses)
        if poses.ndim != 2:
            raise ValueError("poses must be (n, pose_len)")
        n, out = poses.shape[0], {}
        words = {k: np.zeros((n, (self.num_residues(side) + 31) // 32), dtype=np.uint32) for side, k in enumerate(("rec", "lig"))}
        _check(self.lib.ld_complex_contacts(self._h, n, _ptr(poses), poses.shape[1], C.c_double(cutoff), _ptr(words["rec"]),
                                            _ptr(words["lig"])))
        if packed:
            return words
        for side, k in enumerate(("rec", "lig")):
            bits = np.unpackbits(words[k].view(np.uint8), axis=1, bitorder="little")   # little-endian words: bit 32 w + k
            out[k] = bits[:, :self.num_residues(side)].astype(bool)
        return out

    def pair_contacts(self, poses, cutoff=5.0):
        """(n, >= pose_len) poses -> (offsets (n + 1,), keys): the residue pairs of every pose in contact within `cutoff`,
        pose i's as the ascending keys r * num_residues(1) + l in keys[offsets[i]:offsets[i + 1]]
        (ld_complex_pair_contacts: a count call, then the keys)."""
        poses = _f64(poses)
        if poses.ndim != 2:
            raise ValueError("poses must be (n, pose_len)")
        n, total = poses.shape[0], C.c_size_t()
        offsets = np.zeros(n + 1, dtype=np.uint32)
        _check(self.lib.ld_complex_pair_contacts(self._h, n, _ptr(poses), poses.shape[1], C.c_double(cutoff), _ptr(offsets), None, 0,
                                                 C.byref(total)))
        keys = np.zeros(total.value, dtype=np.uint32)
        if total.value:
            _check(self.lib.ld_complex_pair_contacts(self._h, n, _ptr(poses), poses.shape[1], C.c_double(cutoff), _ptr(offsets), _ptr(keys),
                                                     keys.size, C.byref(total)))
        return offsets, keys

    def cluster_fcc(self, poses, scoring, cutoff=5.0, threshold=0.6, min_size=1):
        """One list of poses clustered by the fraction of common contacts (ld_complex_cluster_fcc; lightdock_hip.h,
        "Clustering by common contacts"): poses (n, >= pose_len), scoring (n,) -> dict of cluster_of (n,) in input order
        (-1: unclustered), centres (n,) input indices in creation order (-1 after the last), n_clusters, set_sizes (n,),
        consensus (n,) uint64; fcc_consensus_fraction() turns the last two into fractions."""
        poses, scoring = _f64(poses), _f64(scoring)
        if poses.ndim != 2 or scoring.shape != poses.shape[:1]:
            raise ValueError("poses must be (n, pose_len), scoring (n,)")
        n, k = scoring.shape[0], np.zeros(1, dtype=np.uint32)
        out = {"cluster_of": np.full(n, -1, dtype=np.int32), "centres": np.full(n, -1, dtype=np.int32),
               "set_sizes": np.zeros(n, dtype=np.uint32), "consensus": np.zeros(n, dtype=np.uint64)}
        _check(self.lib.ld_complex_cluster_fcc(self._h, n, _ptr(poses), poses.shape[1], _ptr(scoring), C.c_double(cutoff),
                                               C.c_double(threshold), min_size, _ptr(out["cluster_of"]), _ptr(out["centres"]), _ptr(k),
                                               _ptr(out["set_sizes"]), _ptr(out["consensus"])))
        out["n_clusters"] = int(k[0])
        return out

    def sasa_radii(self, side):
        """The radius of every atom of a side (0 receptor, 1 ligand) in thousandths of an A, 0 for an atom that takes no
        part in the surface: a hydrogen, a deuterium, a membrane bead (ld_complex_sasa_radii)."""
        out = np.zeros(self.num_atoms(side) if side in (0, 1) else 0, dtype=np.uint32)
        _check(self.lib.ld_complex_sasa_radii(self._h, side, _ptr(out)))
        return out

    def sasa(self, poses, probe=1.4, atoms=False):
        """(n, >= pose_len) poses -> {"sums": (n, 4) uint64}: the weighted point counts sum count x E^2 of the receptor
        alone, the receptor in the complex, the ligand alone, the ligand in the complex (ld_complex_sasa; lightdock_hip.h,
        "Solvent-accessible surface"); sasa_area() turns them into A^2.  atoms=True adds "free" and "bound", (n, receptor
        + ligand atoms) uint8: the exposed points, of 128, of every atom in its own molecule and in the complex."""
        poses = _f64(poses)
        if poses.ndim != 2:
            raise ValueError("poses must be (n, pose_len)")
        n = poses.shape[0]
        out = {"sums": np.zeros((n, 4), dtype=np.uint64)}
        if atoms:
            n_atoms = self.num_atoms(0) + self.num_atoms(1)
            out["free"], out["bound"] = np.zeros((n, n_atoms), dtype=np.uint8), np.zeros((n, n_atoms), dtype=np.uint8)
        _check(self.lib.ld_complex_sasa(self._h, n, _ptr(poses), poses.shape[1], C.c_double(probe), _ptr(out["sums"]),
                                        _ptr(out.get("free")), _ptr(out.get("bound"))))
        return out

    def ccs(self, poses, what=2, probe=1.0, cell=0.5, views=False):
        """(n, >= pose_len) poses -> {"ccs": (n,) float64 A^2, "sums": (n,) uint64}: the collision cross-section by the
        projection approximation of the receptor alone (what=0), the posed ligand alone (1) or the complex (2), and the
        covered lattice points summed over the 64 views it is made of, ccs = sums x h^2 / (64 x 10^6) (ld_complex_ccs;
        lightdock_hip.h, "Collision cross-section").  views=True adds "counts", (n, 64) uint32: the points of every view;
        ccs_area() turns them into A^2."""
        poses = _f64(poses)
        if poses.ndim != 2:
            raise ValueError("poses must be (n, pose_len)")
        n = poses.shape[0]
        out = {"sums": np.zeros(n, dtype=np.uint64)}
        if views:
            out["counts"] = np.zeros((n, CCS_VIEWS), dtype=np.uint32)
        _check(self.lib.ld_complex_ccs(self._h, n, _ptr(poses), poses.shape[1], int(what), C.c_double(probe), C.c_double(cell),
                                       _ptr(out.get("counts")), _ptr(out["sums"])))
        out["ccs"] = ccs_area(out["sums"], cell) / CCS_VIEWS
        return out

    def crosslinks(self, poses, links, probe=0.0, cell=1.0, reach=3.0, max_length=35.0, paths=True):
        """(n, >= pose_len) poses, (L, 2) complex atom indices (receptor atoms first, then ligand atoms) -> {"straight2":
        (n, L) uint64 thousandths^2, "straight": (n, L) float64 A, "path": (n, L) uint32 thousandths}: the straight distance of
        every link's two atoms and the length of the shortest path between them over the free nodes of a lattice of step
        `cell`, XLINK_NO_PATH where none of max_length at most exists (ld_complex_crosslinks; lightdock_hip.h, "Cross-links").
        paths=False leaves "path" out and runs no search."""
        poses = _f64(poses)
        if poses.ndim != 2:
            raise ValueError("poses must be (n, pose_len)")
        links = np.ascontiguousarray(links, dtype=np.uint32)
        if links.ndim != 2 or links.shape[1] != 2:
            raise ValueError("links must be (L, 2)")
        n, L = poses.shape[0], links.shape[0]
        out = {"straight2": np.zeros((n, L), dtype=np.uint64)}
        if paths:
            out["path"] = np.zeros((n, L), dtype=np.uint32)
        _check(self.lib.ld_complex_crosslinks(self._h, n, _ptr(poses), poses.shape[1], L, _ptr(links), C.c_double(probe), C.c_double(cell),
                                              C.c_double(reach), C.c_double(max_length), _ptr(out["straight2"]), _ptr(out.get("path"))))
        out["straight"] = np.sqrt(out["straight2"].astype(np.float64)) / 1000.0
        return out

    def saxs_classes(self, side):
        """The scattering class of every atom of a side (0 receptor, 1 ligand): H / D 0, C 1, N 2, O 3, P 4, S 5, and 255
        for an atom that takes no part: another element, a membrane bead (ld_complex_saxs_classes)."""
        out = np.zeros(self.num_atoms(side) if side in (0, 1) else 0, dtype=np.uint8)
        _check(self.lib.ld_complex_saxs_classes(self._h, side, _ptr(out)))
        return out

    def distance_histogram(self, poses, width=0.5, bins=SAXS_MAX_BINS, chunk=0):
        """(n, >= pose_len) poses -> (n, 21, bins) uint32: the pairs of atoms that take part, by pair class and by bin of
        `width` A (a whole number of thousandths, 0.1 .. 2.0) of their distance on the coordinates "%8.3f" prints
        (ld_complex_distance_histogram; lightdock_hip.h, "Small-angle scattering").  A pair beyond the last bin is an
        error.  chunk: the poses whose counts are on the device at a time (ld_complex_saxs_chunk), 0 for as many as
        256 MiB hold; the result does not depend on it."""
        poses = _f64(poses)
        if poses.ndim != 2:
            raise ValueError("poses must be (n, pose_len)")
        out = np.zeros((poses.shape[0], SAXS_PAIR_CLASSES, bins), dtype=np.uint32)
        _check(self.lib.ld_complex_saxs_chunk(self._h, chunk))
        try:
            _check(self.lib.ld_complex_distance_histogram(self._h, poses.shape[0], _ptr(poses), poses.shape[1], saxs_width(width), bins, _ptr(out)))
        finally:
            self.lib.ld_complex_saxs_chunk(self._h, 0)
        return out

    def saxs(self, poses, q, width=0.5, bins=SAXS_MAX_BINS, counts=False, chunk=0):
        """(n, >= pose_len) poses, q (n_q,) in 1 / A -> (n, n_q) intensities by the Debye sum over distance_histogram()'s
        counts, which never leave the device (ld_complex_saxs); counts=True returns (intensities, counts).  chunk as
        distance_histogram()'s."""
        poses, q = _f64(poses), _f64(q).ravel()
        if poses.ndim != 2:
            raise ValueError("poses must be (n, pose_len)")
        n = poses.shape[0]
        out = np.zeros((n, q.size))
        hist = np.zeros((n, SAXS_PAIR_CLASSES, bins), dtype=np.uint32) if counts else None
        _check(self.lib.ld_complex_saxs_chunk(self._h, chunk))
        try:
            _check(self.lib.ld_complex_saxs(self._h, n, _ptr(poses), poses.shape[1], saxs_width(width), bins, _ptr(q), q.size, _ptr(out), _ptr(hist)))
        finally:
            self.lib.ld_complex_saxs_chunk(self._h, 0)
        return (out, hist) if counts else out

    def density_fit(self, poses, density, sigma, chunk=0):
        """(n, >= pose_len) poses, a Density, sigma in whole thousandths -> {"s", "ss", "se", "inside_sum" (n,) uint64,
        "outside" (n,) uint32}: the exact sums of every pose's simulated density against the map (ld_complex_density_fit).
        chunk: the poses on the device at a time (ld_complex_density_chunk), 0 for as many as 256 MiB hold; the words do
        not depend on it."""
        poses = _f64(poses)
        if poses.ndim != 2:
            raise ValueError("poses must be (n, pose_len)")
        rows = np.zeros(poses.shape[0], dtype=DENSITY_SUMS)
        _check(self.lib.ld_complex_density_chunk(self._h, chunk))
        try:
            _check(self.lib.ld_complex_density_fit(self._h, density._h, poses.shape[0], _ptr(poses), poses.shape[1], int(sigma), _ptr(rows)))
        finally:
            self.lib.ld_complex_density_chunk(self._h, 0)
        return {k: rows[k].copy() for k in ("s", "ss", "se", "inside_sum", "outside")}

    def simulate_density(self, poses, density, sigma, chunk=0):
        """(n, nz, ny, nx) uint32: the voxels density_fit() sums (ld_complex_simulate_density); at most 256 MiB a call."""
        poses = _f64(poses)
        if poses.ndim != 2:
            raise ValueError("poses must be (n, pose_len)")
        out = np.zeros((poses.shape[0],) + tuple(density.shape), dtype=np.uint32)
        _check(self.lib.ld_complex_density_chunk(self._h, chunk))
        try:
            _check(self.lib.ld_complex_simulate_density(self._h, density._h, poses.shape[0], _ptr(poses), poses.shape[1], int(sigma), _ptr(out)))
        finally:
            self.lib.ld_complex_density_chunk(self._h, 0)
        return out

    def write_pdb(self, pose, path):
        pose = _f64(pose).ravel()
        if pose.size != self.pose_len:
            raise ValueError("pose must have %d values" % self.pose_len)
        _check(self.lib.ld_complex_write_pdb(self._h, _ptr(pose), os.fsencode(path)))

    def set_reference(self, ref_receptor_pdb, ref_ligand_pdb, contact_cutoff=5.0, interface_cutoff=10.0):
        """The bound complex assess() measures against (ld_complex_set_reference; lightdock_hip.h, "Model quality").
        A refusal leaves the complex without a reference."""
        _check(self.lib.ld_complex_set_reference(self._h, os.fsencode(ref_receptor_pdb), os.fsencode(ref_ligand_pdb),
                                                 C.c_double(contact_cutoff), C.c_double(interface_cutoff)))

    def reference_counts(self):
        """dict: matched_rec, matched_lig, native_pairs, rec_fit, lig_fit, interface_fit."""
        out = np.zeros(6, dtype=np.uint32)
        _check(self.lib.ld_complex_reference_counts(self._h, _ptr(out)))
        return dict(zip(("matched_rec", "matched_lig", "native_pairs", "rec_fit", "lig_fit", "interface_fit"), (int(v) for v in out)))

    def native_pairs(self):
        """(n_native, 2) residue indices (receptor, ligand) of the reference's native pairs, sorted."""
        out = np.zeros((self.reference_counts()["native_pairs"], 2), dtype=np.uint32)
        _check(self.lib.ld_complex_native_pairs(self._h, _ptr(out)))
        return out

    def assess(self, poses):
        """(n, >= pose_len) poses -> {"kept": native pairs in contact, "fnat", "lrmsd", "irmsd"} per pose (ld_complex_assess)."""
        poses = _f64(poses)
        if poses.ndim != 2:
            raise ValueError("poses must be (n, pose_len)")
        n = poses.shape[0]
        kept, lrmsd, irmsd = np.zeros(n, dtype=np.uint32), np.zeros(n), np.zeros(n)
        n_native = self.reference_counts()["native_pairs"]
        _check(self.lib.ld_complex_assess(self._h, n, _ptr(poses), poses.shape[1], _ptr(kept), _ptr(lrmsd), _ptr(irmsd)))
        return {"kept": kept, "fnat": kept / float(n_native), "lrmsd": lrmsd, "irmsd": irmsd}


def _sets(offsets, keys):
    offsets, keys = np.ascontiguousarray(offsets, dtype=np.uint32), np.ascontiguousarray(keys, dtype=np.uint32)
    if offsets.ndim != 1 or offsets.size < 1 or keys.ndim != 1:
        raise ValueError("offsets must be (n + 1,), keys (total,)")
    if keys.size < int(offsets.max()):
        raise ValueError("offsets point beyond the keys")
    return offsets, keys


def fcc_common(offsets, keys):
    """Sets in CSR form (set i: the strictly ascending keys[offsets[i]:offsets[i + 1]]) -> (n, n) uint32, the number of
    keys every two sets share, the diagonal their sizes (ld_fcc_common)."""
    offsets, keys = _sets(offsets, keys)
    n = offsets.size - 1
    out = np.zeros((n, n), dtype=np.uint32)
    _check(load_library().ld_fcc_common(n, _ptr(offsets), _ptr(keys), _ptr(out)))
    return out


def fcc_cluster(offsets, keys, scoring, threshold=0.6, min_size=1):
    """Complex.cluster_fcc's rule on the caller's sets (ld_fcc_cluster) -> dict of cluster_of, centres, n_clusters,
    set_sizes, consensus."""
    offsets, keys = _sets(offsets, keys)
    scoring = _f64(scoring)
    n, k = offsets.size - 1, np.zeros(1, dtype=np.uint32)
    if scoring.shape != (n,):
        raise ValueError("scoring must be (n,)")
    out = {"cluster_of": np.full(n, -1, dtype=np.int32), "centres": np.full(n, -1, dtype=np.int32),
           "consensus": np.zeros(n, dtype=np.uint64)}
    _check(load_library().ld_fcc_cluster(n, _ptr(offsets), _ptr(keys), _ptr(scoring), C.c_double(threshold), min_size,
                                         _ptr(out["cluster_of"]), _ptr(out["centres"]), _ptr(k), _ptr(out["consensus"])))
    out["n_clusters"] = int(k[0])
    out["set_sizes"] = np.diff(offsets.astype(np.int64)).astype(np.uint32)
    return out


def fcc_consensus_fraction(consensus, set_sizes):
    """consensus_i / (s_i * n), and 0 for an empty set: how often, on average, a pose's pairs recur over the list."""
    consensus, sizes = np.asarray(consensus, dtype=np.float64), np.asarray(set_sizes, dtype=np.float64)
    return np.where(sizes > 0, consensus / np.maximum(sizes * max(1, sizes.size), 1.0), 0.0)


def fcc_last_kernel_ms():
    ms = C.c_double()
    _check(load_library().ld_fcc_last_kernel_ms(C.byref(ms)))
    return ms.value


SASA_POINTS = 128


def sasa_directions():
    """The (128, 3) int32 table of the surface rule: rint(2^20 x golden-spiral unit vector) (ld_sasa_directions)."""
    out = np.zeros((SASA_POINTS, 3), dtype=np.int32)
    _check(load_library().ld_sasa_directions(_ptr(out)))
    return out


def sasa_area(weighted):
    """Weighted point counts (count x E^2 in thousandths^2: sasa()'s sums, their differences, an atom's count times its
    squared expanded radius) -> A^2: x 4 pi / (128 x 10^6)."""
    return np.asarray(weighted, dtype=np.float64) * (4.0 * np.pi / (SASA_POINTS * 1e6))


XLINK_NO_PATH = 0xffffffff             # LD_XLINK_NO_PATH

CCS_VIEWS = 64


def ccs_frames():
    """The (64, 2, 3) int32 table of the cross-section rule: rint(2^20 x in-plane axis), A then B of every view (ld_ccs_frames)."""
    out = np.zeros((CCS_VIEWS, 2, 3), dtype=np.int32)
    _check(load_library().ld_ccs_frames(_ptr(out)))
    return out


def ccs_area(points, cell=0.5):
    """Covered lattice points of a view (ccs()'s counts) -> the view's area in A^2: x h^2 / 10^6, h = rint(1000 cell)."""
    h = int(np.rint(1000.0 * cell))
    return np.asarray(points, dtype=np.float64) * float(h * h) / 1e6


def saxs_form_factors(q):
    """q (n_q,) in 1 / A -> (n_q, 6): the form factor of H, C, N, O, P, S less its displaced solvent (ld_saxs_form_factors)."""
    q = _f64(q).ravel()
    out = np.zeros((q.size, SAXS_CLASSES))
    _check(load_library().ld_saxs_form_factors(_ptr(q), q.size, _ptr(out)))
    return out


def saxs_sinc(q, width=0.5, bins=SAXS_MAX_BINS):
    """(n_q, bins): sin(x) / x at x = q_j r_k, r_k = (k + 0.5) width, and 1 at x == 0 (ld_saxs_sinc)."""
    q = _f64(q).ravel()
    out = np.zeros((q.size, bins))
    _check(load_library().ld_saxs_sinc(_ptr(q), q.size, saxs_width(width), bins, _ptr(out)))
    return out


def saxs_debye(counts, class_atoms, q, width=0.5):
    """counts (n, 21, bins) uint32, class_atoms (6,) -> (n, n_q): the Debye sum on the GPU (ld_saxs_debye)."""
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    class_atoms, q = np.ascontiguousarray(class_atoms, dtype=np.uint32), _f64(q).ravel()
    if counts.ndim != 3 or counts.shape[1] != SAXS_PAIR_CLASSES or class_atoms.shape != (SAXS_CLASSES,):
        raise ValueError("counts must be (n, 21, bins), class_atoms (6,)")
    out = np.zeros((counts.shape[0], q.size))
    _check(load_library().ld_saxs_debye(counts.shape[0], _ptr(counts), saxs_width(width), counts.shape[2], _ptr(class_atoms), _ptr(q), q.size, _ptr(out)))
    return out


def saxs_fit(intensity, i_exp, sigma):
    """intensity (n, n_q), i_exp and sigma (n_q,) -> (scale (n,), chi2 (n,)) (ld_saxs_fit)."""
    intensity, i_exp, sigma = _f64(intensity), _f64(i_exp).ravel(), _f64(sigma).ravel()
    if intensity.ndim != 2 or i_exp.shape != intensity.shape[1:] or sigma.shape != i_exp.shape:
        raise ValueError("intensity must be (n, n_q), i_exp and sigma (n_q,)")
    n = intensity.shape[0]
    scale, chi2 = np.zeros(n), np.zeros(n)
    _check(load_library().ld_saxs_fit(n, i_exp.size, _ptr(intensity), _ptr(i_exp), _ptr(sigma), _ptr(scale), _ptr(chi2)))
    return scale, chi2


ANM_CUTOFF = 15.0


def anm_nodes(pdb_path):
    """The node atom of every residue of a PDB file (ld_anm_nodes; lightdock_hip.h, "Normal modes"): indices into the
    file's ATOM / HETATM records, one a residue, in file order.  Host only."""
    lib = load_library()
    n = C.c_size_t()
    _check(lib.ld_anm_nodes(os.fsencode(pdb_path), None, C.byref(n)))
    out = np.zeros(n.value, dtype=np.uint32)
    _check(lib.ld_anm_nodes(os.fsencode(pdb_path), _ptr(out), C.byref(n)))
    return out


def anm_modes_xyz(node_xyz, n_modes, cutoff=ANM_CUTOFF):
    """(eigenvalues (k,), unit modes (k, nodes, 3)) of an anisotropic network on raw node coordinates (ld_anm_modes_xyz)."""
    xyz = _f64(node_xyz).reshape(-1, 3)
    k = max(0, int(n_modes))
    modes, eig = np.zeros((k, xyz.shape[0], 3)), np.zeros(k)
    _check(load_library().ld_anm_modes_xyz(_ptr(xyz), xyz.shape[0], k, C.c_double(cutoff), _ptr(modes), _ptr(eig)))
    return eig, modes


def anm_modes(pdb_path, n_modes, cutoff=ANM_CUTOFF, rmsd=0.0):
    """(eigenvalues (k,), modes (k, atoms, 3) in file order) of a PDB file: what lightdock_rec.nm.npy holds (ld_anm_modes).
    rmsd = 0: every mode of norm 1; rmsd > 0: the library's amplitude rule."""
    lib = load_library()
    try:
        with open(pdb_path, errors="replace") as f:
            atoms = sum(1 for line in f if line.startswith("ATOM  ") or line.startswith("HETATM"))
    except OSError:   # the library says why (LD_ERR_IO) before it writes anything
        atoms = 0
    k = max(0, int(n_modes))
    modes, eig = np.zeros((k, atoms, 3)), np.zeros(k)
    _check(lib.ld_anm_modes(os.fsencode(pdb_path), k, C.c_double(cutoff), C.c_double(rmsd), _ptr(modes), _ptr(eig)))
    return eig, modes


def anm_last_kernel_ms():
    """The device work of this thread's last anm_modes / anm_modes_xyz, in ms (HIP events)."""
    ms = C.c_double()
    _check(load_library().ld_anm_last_kernel_ms(C.byref(ms)))
    return ms.value


KEEP_HYDROGENS, KEEP_OXT, KEEP_WATERS = 1, 2, 4


def _i32(a, columns):
    return np.ascontiguousarray(a, dtype=np.int32).reshape(-1, columns)


def swarm_diameter2(xyz):
    """max |x_i - x_j|^2 of (n, 3) int32 thousandths, exact (ld_swarm_diameter2; lightdock_hip.h, "Preparing a run")."""
    xyz = _i32(xyz, 3)
    out = C.c_uint64()
    _check(load_library().ld_swarm_diameter2(_ptr(xyz), xyz.shape[0], C.byref(out)))
    return out.value


def swarm_shell_count(atoms, bead=None, spacing=2000):
    """(candidates, lattice nodes) of ld_swarm_shell's count-only call."""
    atoms = _i32(atoms, 4)
    flags = None if bead is None else np.ascontiguousarray(bead, dtype=np.uint8)
    count, nodes = C.c_size_t(), C.c_uint64()
    _check(load_library().ld_swarm_shell(_ptr(atoms), _ptr(flags), atoms.shape[0], int(spacing), None, 0, C.byref(count), C.byref(nodes)))
    return count.value, nodes.value


def swarm_shell(atoms, bead=None, spacing=2000, lattice_nodes=False):
    """The shell candidates of (n, 4) int32 atoms x y z E, `bead` flagging those that attract no node: (count, 3) int32 in
    lexicographic order (ld_swarm_shell, the count-only call and then the filling one).  lattice_nodes=True: (candidates,
    the number of lattice nodes tested)."""
    atoms = _i32(atoms, 4)
    flags = None if bead is None else np.ascontiguousarray(bead, dtype=np.uint8)
    count, nodes = swarm_shell_count(atoms, flags, spacing)
    out = np.zeros((count, 3), dtype=np.int32)
    got = C.c_size_t()
    _check(load_library().ld_swarm_shell(_ptr(atoms), _ptr(flags), atoms.shape[0], int(spacing), _ptr(out), count, C.byref(got), None))
    return (out[:got.value], nodes) if lattice_nodes else out[:got.value]


def swarm_centres(points, max_centres, cover=0):
    """Farthest-point sampling of (n, 3) int32 points: (indices uint32, gap2 uint64) in the order picked (ld_swarm_centres)."""
    points = _i32(points, 3)
    room = max(1, min(int(max_centres), points.shape[0]))
    index, gap2, n = np.zeros(room, dtype=np.uint32), np.zeros(room, dtype=np.uint64), C.c_size_t()
    _check(load_library().ld_swarm_centres(_ptr(points), points.shape[0], int(max_centres), int(cover), _ptr(index), _ptr(gap2), C.byref(n)))
    return index[:n.value], gap2[:n.value]


def initial_poses(seed, glowworms, swarm, centre, first=0, n=None, radius=10.0, rec_points=None, lig_points=None, anm_rec=0,
                  anm_lig=0):
    """(rows (n, 7 + anm_rec + anm_lig), draws (n,) uint64) of glowworms first .. first + n - 1 of one swarm
    (ld_initial_poses; host only)."""
    n = glowworms - first if n is None else n
    centre = _f64(centre).reshape(3)
    rec = np.zeros((0, 3)) if rec_points is None else _f64(rec_points).reshape(-1, 3)
    lig = np.zeros((0, 3)) if lig_points is None else _f64(lig_points).reshape(-1, 3)
    rows, draws = np.zeros((max(0, n), 7 + anm_rec + anm_lig)), np.zeros(max(0, n), dtype=np.uint64)
    _check(load_library().ld_initial_poses(seed, glowworms, swarm, first, n, _ptr(centre), C.c_double(radius), _ptr(rec), rec.shape[0],
                                           _ptr(lig), lig.shape[0], anm_rec, anm_lig, _ptr(rows), _ptr(draws)))
    return rows, draws


def prepare_pdb(in_path, out_path, keep_h=False, keep_oxt=False, keep_waters=False):
    """Writes the cleaned, centred copy of a PDB file; (atoms written, the mean subtracted in A) (ld_prepare_pdb; host only)."""
    flags = (KEEP_HYDROGENS if keep_h else 0) | (KEEP_OXT if keep_oxt else 0) | (KEEP_WATERS if keep_waters else 0)
    atoms, centre = C.c_size_t(), np.zeros(3)
    _check(load_library().ld_prepare_pdb(os.fsencode(in_path), os.fsencode(out_path), flags, C.byref(atoms), _ptr(centre)))
    return atoms.value, centre


def refine_plan(pose_len, n, stride=None, iterations=1, slice_poses=0):
    """K, the poses per pass and the device workspace of a refinement call (ld_refine_plan; host only)."""
    trials, slice_out, ws = C.c_size_t(), C.c_size_t(), C.c_size_t()
    _check(load_library().ld_refine_plan(pose_len, n, pose_len if stride is None else stride, iterations, slice_poses,
                                         C.byref(trials), C.byref(slice_out), C.byref(ws)))
    return {"trials": trials.value, "slice": slice_out.value, "workspace_bytes": ws.value}


def _refine_state(state, n):
    """The arrays of a state dict (REFINE_STATE) as contiguous arrays of n, and the struct that points at them."""
    arrays = {k: np.ascontiguousarray(state[k], dtype=dt).copy() for k, dt in REFINE_STATE}
    if any(a.shape != (n,) for a in arrays.values()):
        raise ValueError("one state entry per pose")
    return arrays, _RefineState(*[_ptr(arrays[k]) for k, _ in REFINE_STATE])


def refine_trials(poses, pose_len, state, trials, active=None):
    """refine_trials alone on caller-given state (ld_refine_trials; a test entry).  poses: (n, stride); trials: (n, K,
    trial_stride), whose rows come back with the trial rows written into them.  Returns (trials, active (n, K) uint8)."""
    poses = _f64(poses)
    n, K = poses.shape[0], 12 + 2 * (pose_len - 7)
    trials = _f64(trials).copy()
    if trials.shape[:2] != (n, K):
        raise ValueError("trials must be (n, K, trial_stride)")
    active = np.zeros((n, K), dtype=np.uint8) if active is None else np.ascontiguousarray(active, dtype=np.uint8).copy()
    _, struct = keep = _refine_state(state, n)
    _check(load_library().ld_refine_trials(n, pose_len, _ptr(poses), poses.shape[1], C.byref(struct), _ptr(trials),
                                           trials.shape[2], _ptr(active)))
    del keep
    return trials, active


def refine_select(poses, pose_len, state, energies, max_halvings):
    """refine_select alone on caller-given state and energies (ld_refine_select; a test entry).  Returns (poses, state,
    history (n,) int16); the inputs are not changed."""
    poses = _f64(poses).copy()
    n = poses.shape[0]
    energies = _f64(energies)
    if energies.shape != (n, 12 + 2 * (pose_len - 7)):
        raise ValueError("energies must be (n, K)")
    arrays, struct = _refine_state(state, n)
    history = np.zeros(n, dtype=np.int16)
    _check(load_library().ld_refine_select(n, pose_len, _ptr(poses), poses.shape[1], C.byref(struct), _ptr(energies),
                                           max_halvings, _ptr(history)))
    return poses, arrays, history


def setup_last_kernel_ms():
    """The device work of this thread's last swarm_diameter2 / swarm_shell / swarm_centres call, in ms (HIP events)."""
    ms = C.c_double()
    _check(load_library().ld_setup_last_kernel_ms(C.byref(ms)))
    return ms.value


def cli_main(argv):
    """The reference command line, in process (src/bin/lightdock-rust.rs:77-333)."""
    args = [os.fsencode(a) for a in argv]
    arr = (C.c_char_p * len(args))(*args)
    return load_library().ld_cli_main(len(args), arr)


from . import multi, synth  # noqa: E402,F401
