// capi.cpp -- extern "C" surface declared in include/lightdock_hip.h.
//
// Every call catches ld::Error and turns it into an ld_status plus a thread-local
// message, which is how this library reports what the reference reports by panicking.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <new>
#include <string>
#include <vector>

#include "anm.hpp"
#include "complex.hpp"
#include "emfit.hpp"
#include "fcc.hpp"
#include "gso.hpp"
#include "host/cli.hpp"
#include "host/docking_model.hpp"
#include "host/error.hpp"
#include "host/initial_poses.hpp"
#include "host/io.hpp"
#include "host/prepare_pdb.hpp"
#include "host/refine_plan.hpp"
#include "host/spatial_order.hpp"
#include "kernels/ccs.hpp"
#include "lightdock_hip.h"
#include "prepare.hpp"
#include "refine.hpp"
#include "saxs.hpp"
#include "scorer.hpp"

namespace {

thread_local std::string g_last_error;

int fail(ld_status code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

template <typename F>
int guarded(F &&f) {
    try {
        f();
        return LD_OK;
    } catch (const ld::Error &e) {
        return fail(e.code(), e.what());
    } catch (const std::bad_alloc &) {
        return fail(LD_ERR_NOMEM, "out of host memory");
    } catch (const std::exception &e) {
        return fail(LD_ERR_INVALID, e.what());
    }
}

std::vector<std::string> to_strings(const char *const *list, size_t n) {
    std::vector<std::string> out;
    for (size_t i = 0; i < n; i++)
        if (list && list[i]) out.emplace_back(list[i]);
    return out;
}

}  // namespace

extern "C" {

const char *ld_last_error(void) { return g_last_error.c_str(); }
const char *ld_version(void) { return "lightdock-hip 0.1.0 (gfx950; path of lightdock-rust 0.3.2)"; }

int ld_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int ld_init(int device) {
    return guarded([&] {
        int n = ld_device_count();
        if (n <= 0) throw ld::Error(LD_ERR_DEVICE, "no HIP device available: the pose-energy path has no CPU fallback");
        int dev = device;
        if (dev < 0) {
            const char *e = std::getenv("LIGHTDOCK_DEVICE");
            dev = e ? std::atoi(e) : 0;
        }
        if (dev >= n) throw ld::Error(LD_ERR_DEVICE, "device index out of range");
        ld::hip_check(hipSetDevice(dev), "hipSetDevice");
    });
}

ld_scorer *ld_scorer_create(const ld_scorer_desc *desc) {
    ld_scorer *s = nullptr;
    int rc = guarded([&] {
        if (!desc) throw ld::Error(LD_ERR_INVALID, "ld_scorer_create: null descriptor");
        s = new ld_scorer(*desc);
    });
    return rc == LD_OK ? s : nullptr;
}

ld_scorer *ld_scorer_create_from_pdb(int method, const char *receptor_pdb, const char *ligand_pdb,
                                     const char *const *rec_active, size_t n_rec_active,
                                     const char *const *rec_passive, size_t n_rec_passive, const double *rec_nmodes,
                                     size_t rec_nmodes_len, size_t rec_num_anm, const char *const *lig_active,
                                     size_t n_lig_active, const char *const *lig_passive, size_t n_lig_passive,
                                     const double *lig_nmodes, size_t lig_nmodes_len, size_t lig_num_anm, int use_anm,
                                     const double *potential) {
    ld_scorer *s = nullptr;
    int rc = guarded([&] {
        if (!receptor_pdb || !ligand_pdb) throw ld::Error(LD_ERR_INVALID, "PDB path missing");
        if (method != LD_METHOD_DFIRE && method != LD_METHOD_DNA && method != LD_METHOD_PYDOCK)
            throw ld::Error(LD_ERR_UNSUPPORTED, "Error: method not supported");
        ld::Structure rec = ld::read_pdb(receptor_pdb);
        ld::Structure lig = ld::read_pdb(ligand_pdb);
        std::vector<double> rnm, lnm;
        if (rec_nmodes && rec_nmodes_len) rnm.assign(rec_nmodes, rec_nmodes + rec_nmodes_len);
        if (lig_nmodes && lig_nmodes_len) lnm.assign(lig_nmodes, lig_nmodes + lig_nmodes_len);
        if (use_anm) {  // src/bin/lightdock-rust.rs:233,250
            if (rec_num_anm > 0 && rnm.size() != rec.atom_count() * 3 * rec_num_anm)
                throw ld::Error(LD_ERR_INVALID, "Number of read ANM in receptor does not correspond to the number of atoms");
            if (lig_num_anm > 0 && lnm.size() != lig.atom_count() * 3 * lig_num_anm)
                throw ld::Error(LD_ERR_INVALID, "Number of read ANM in ligand does not correspond to the number of atoms");
        }
        ld::DockingModel rm = ld::build_docking_model(method, rec, to_strings(rec_active, n_rec_active),
                                                      to_strings(rec_passive, n_rec_passive), rnm, rec_num_anm);
        ld::DockingModel lm = ld::build_docking_model(method, lig, to_strings(lig_active, n_lig_active),
                                                      to_strings(lig_passive, n_lig_passive), lnm, lig_num_anm);
        ld_scorer_desc d;
        std::memset(&d, 0, sizeof d);
        d.method = method;
        d.use_anm = use_anm;
        d.receptor = rm.view();
        d.ligand = lm.view();
        d.potential = potential;
        s = new ld_scorer(d);
    });
    return rc == LD_OK ? s : nullptr;
}

void ld_scorer_destroy(ld_scorer *s) { delete s; }

/* ---- host-only model builder ------------------------------------------------------------ */
struct ld_model {
    ld::DockingModel model;
};

ld_model *ld_model_from_pdb(int method, const char *pdb_path, const char *const *active, size_t n_active,
                            const char *const *passive, size_t n_passive, const double *nmodes, size_t nmodes_len,
                            size_t num_anm) {
    ld_model *m = nullptr;
    int rc = guarded([&] {
        if (!pdb_path) throw ld::Error(LD_ERR_INVALID, "PDB path missing");
        ld::Structure st = ld::read_pdb(pdb_path);
        std::vector<double> nm;
        if (nmodes && nmodes_len) nm.assign(nmodes, nmodes + nmodes_len);
        if (num_anm > 0 && !nm.empty() && nm.size() != st.atom_count() * 3 * num_anm)
            throw ld::Error(LD_ERR_INVALID, "Number of read ANM does not correspond to the number of atoms");
        m = new ld_model{ld::build_docking_model(method, st, to_strings(active, n_active), to_strings(passive, n_passive),
                                                 nm, num_anm)};
    });
    return rc == LD_OK ? m : nullptr;
}
int ld_model_view(const ld_model *m, ld_molecule *out) {
    return guarded([&] {
        if (!m || !out) throw ld::Error(LD_ERR_INVALID, "null argument");
        *out = m->model.view();
    });
}
void ld_model_destroy(ld_model *m) { delete m; }
size_t ld_model_num_residues(const ld_model *m) { return m ? m->model.residue_ids.size() : 0; }
int ld_model_residue_id(const ld_model *m, size_t index, char *buf, size_t buf_len) {
    return guarded([&] {
        if (!m || !buf) throw ld::Error(LD_ERR_INVALID, "null argument");
        if (index >= m->model.residue_ids.size()) throw ld::Error(LD_ERR_INVALID, "residue index out of range");
        const std::string &id = m->model.residue_ids[index];
        if (id.size() + 1 > buf_len) throw ld::Error(LD_ERR_INVALID, "buffer too short for the residue id");
        std::memcpy(buf, id.c_str(), id.size() + 1);
    });
}
int ld_model_residue_of_atom(const ld_model *m, uint32_t *out) {
    return guarded([&] {
        if (!m || !out) throw ld::Error(LD_ERR_INVALID, "null argument");
        std::memcpy(out, m->model.residue_of_atom.data(), m->model.residue_of_atom.size() * sizeof(uint32_t));
    });
}

int ld_dfire_bin_lut(uint8_t *lut_out, double *steps_out, double *interface_d2_out) {
    return guarded([&] {
        const ld::DfireBinning t = ld::build_dfire_binning();
        if (lut_out) std::memcpy(lut_out, t.lut.data(), 901);
        if (steps_out) std::memcpy(steps_out, t.step.data(), 21 * sizeof(double));
        if (interface_d2_out) *interface_d2_out = ld::dfire_interface_d2();
    });
}
int ld_dfire_packed_lut(int cells_per_unit, double ubound, uint32_t *words_out, double *eps_out) {
    return guarded([&] {
        if (cells_per_unit != 1 && cells_per_unit != 2) throw ld::Error(LD_ERR_INVALID, "cells_per_unit must be 1 or 2");
        if (!(ubound > 0.0)) throw ld::Error(LD_ERR_INVALID, "ubound must be positive");
        const double eps = (double)std::nextafter((float)ld::dfire_f32_error_bound(ubound, cells_per_unit), INFINITY);
        const std::vector<uint32_t> words = ld::build_packed_lut(cells_per_unit, eps);
        if (words_out) std::memcpy(words_out, words.data(), words.size() * sizeof(uint32_t));
        if (eps_out) *eps_out = eps;
    });
}
int ld_dfire_bm_lut(double ubound, double lig_extent, uint8_t *codes_out, double *eps_cells_out) {
    return guarded([&] {
        if (!(ubound > 0.0) || !(lig_extent >= 0.0)) throw ld::Error(LD_ERR_INVALID, "ubound must be positive, lig_extent non-negative");
        const double eps = ld::dfire_bm_error_bound(ubound, lig_extent);
        const std::vector<uint8_t> codes = ld::build_bm_lut(eps);
        if (codes_out) std::memcpy(codes_out, codes.data(), codes.size());
        if (eps_cells_out) *eps_cells_out = eps;
    });
}
int ld_dfire_route_frames(const double *rec_xyz, const uint32_t *rec_types, size_t n_rec, const double *lig_xyz, size_t n_lig, int anm,
                          double *bm_out, double *packed_out) {
    return guarded([&] {
        if (!rec_xyz || !n_rec || !lig_xyz || !n_lig) throw ld::Error(LD_ERR_INVALID, "coordinates of both molecules");
        ld_molecule rec{}, lig{};
        rec.n_atoms = n_rec;
        rec.coordinates = rec_xyz;
        lig.n_atoms = n_lig;
        lig.coordinates = lig_xyz;
        if (bm_out) {
            double sub_axis = 0.0, sub_diag = 0.0;
            if (rec_types) {   // the receptor in the scorer's tile order, as bm_accepts measures its subtiles
                const std::vector<uint32_t> order = ld::dfire_tile_layout(rec_xyz, rec_types, n_rec).order;
                std::vector<double> x(order.size(), 0.0), y(order.size(), 0.0), z(order.size(), 0.0);
                std::vector<uint32_t> type(order.size(), std::numeric_limits<uint32_t>::max());
                for (size_t i = 0; i < order.size(); i++) {
                    if (order[i] >= n_rec) continue;
                    x[i] = rec_xyz[3 * (size_t)order[i]];
                    y[i] = rec_xyz[3 * (size_t)order[i] + 1];
                    z[i] = rec_xyz[3 * (size_t)order[i] + 2];
                    type[i] = rec_types[order[i]];
                }
                ld::dfire_bm_subtile_extents(x, y, z, type, &sub_axis, &sub_diag);
            }
            ld::BmFrame f;
            const bool takes = ld::dfire_bm_frame(rec, lig, anm != 0, sub_axis, sub_diag, &f);
            const double row[9] = {f.centre[0], f.centre[1], f.centre[2], f.ubound, f.extent, f.eps, takes ? 1.0 : 0.0, sub_axis, sub_diag};
            std::memcpy(bm_out, row, sizeof row);
        }
        if (packed_out) {
            ld::PackedFrame f;
            const bool takes = ld::packed_accepts(rec, &f);
            const double row[8] = {f.centre[0], f.centre[1], f.centre[2], f.kappa, f.ubound, f.eps, (double)f.cells, takes ? 1.0 : 0.0};
            std::memcpy(packed_out, row, sizeof row);
        }
    });
}
int ld_dfire_bm_fix_scale(const double *rec_xyz, size_t n_rec, double reach, double table_vmax, uint64_t *reach_count_out,
                          int *extra_bits_out, double *scale_out) {
    return guarded([&] {
        if ((!rec_xyz && n_rec) || !(reach > 0.0) || !(table_vmax >= 0.0)) throw ld::Error(LD_ERR_INVALID, "coordinates, a positive reach and a non-negative table maximum");
        const size_t count = ld::dfire_bm_reach_count(rec_xyz, n_rec, reach);
        int extra = 0;
        const double scale = ld::dfire_bm_fix_scale(table_vmax, count, &extra);
        if (reach_count_out) *reach_count_out = (uint64_t)count;
        if (extra_bits_out) *extra_bits_out = extra;
        if (scale_out) *scale_out = scale;
    });
}
int ld_dfire_bm_workspace(size_t n_rt, size_t n_lt, size_t cap, size_t sets, size_t waves, int flags, const char **names_out,
                          uint64_t *rows_out) {
    static_assert(ld::kBmRegions == 22, "the region count the header states");
    return guarded([&] {
        if (!n_rt || !n_lt || !cap || sets < 1 || sets > 2) throw ld::Error(LD_ERR_INVALID, "tiles and a pass size, one or two sets");
        ld::BmShape s;
        s.n_rt = n_rt;
        s.n_lt = n_lt;
        s.cap = cap;
        s.sets = sets;
        s.waves = waves;
        s.anm = (flags & 1) != 0;
        s.counts = (flags & 2) != 0;
        s.debug = (flags & 4) != 0;
        const ld::BmLayout L = ld::bm_layout(s);
        for (int r = 0; r < ld::kBmRegions; r++) {
            const ld::BmRegion &g = L.region[r];
            if (names_out) {
                names_out[2 * r] = g.name;
                names_out[2 * r + 1] = g.buffer_name;
            }
            if (rows_out) {
                const uint64_t row[5] = {(uint64_t)g.buffer, L.buffer_bytes[g.buffer], g.base, g.stride, g.bytes};
                std::memcpy(rows_out + 5 * r, row, sizeof row);
            }
        }
    });
}
size_t ld_spatial_tile_order(const double *xyz, size_t n, uint32_t *order_out) {
    size_t len = 0;
    guarded([&] {
        if (!xyz && n) throw ld::Error(LD_ERR_INVALID, "null coordinates");
        const std::vector<uint32_t> order = ld::spatial_tile_order(xyz, n);
        if (order_out) std::memcpy(order_out, order.data(), order.size() * sizeof(uint32_t));
        len = order.size();
    });
    return len;
}
size_t ld_dfire_tile_layout(const double *xyz, const uint32_t *dfire_types, size_t n, uint32_t *order_out,
                            uint32_t *type_perm_out) {
    size_t len = 0;
    guarded([&] {
        if ((!xyz || !dfire_types) && n) throw ld::Error(LD_ERR_INVALID, "null coordinates / types");
        const ld::DfireTileLayout layout = ld::dfire_tile_layout(xyz, dfire_types, n);
        if (order_out) std::memcpy(order_out, layout.order.data(), layout.order.size() * sizeof(uint32_t));
        if (type_perm_out) std::memcpy(type_perm_out, layout.type_perm.data(), layout.type_perm.size() * sizeof(uint32_t));
        len = layout.order.size();
    });
    return len;
}
void ld_stdrng_key(uint64_t seed, uint32_t key_out[8]) { ld::stdrng_key_from_seed(seed, key_out); }

int ld_load_dcparams(const char *path, double *out) {
    return guarded([&] {
        if (!path || !out) throw ld::Error(LD_ERR_INVALID, "ld_load_dcparams: null argument");
        std::vector<double> t = ld::load_dcparams(path);
        std::memcpy(out, t.data(), sizeof(double) * LD_DFIRE_TABLE_LEN);
    });
}

size_t ld_scorer_num_atoms(const ld_scorer *s, int side) { return s ? s->impl.num_atoms(side) : 0; }
size_t ld_scorer_pose_len(const ld_scorer *s) { return s ? s->impl.pose_len() : 0; }
int ld_scorer_method(const ld_scorer *s) { return s ? s->impl.method() : LD_ERR_INVALID; }

int ld_scorer_model_arrays(const ld_scorer *s, int side, double *coordinates, uint32_t *dfire_types, double *ele_charges,
                           double *vdw_charges, double *vdw_radii) {
    return guarded([&] {
        if (!s) throw ld::Error(LD_ERR_INVALID, "null scorer");
        const ld::HostMolecule &m = s->impl.host_molecule(side);
        auto put = [](auto *dst, const auto &src) {
            if (dst && !src.empty()) std::memcpy(dst, src.data(), src.size() * sizeof(src[0]));
        };
        put(coordinates, m.coordinates);
        put(dfire_types, m.dfire_types);
        put(ele_charges, m.ele_charges);
        put(vdw_charges, m.vdw_charges);
        put(vdw_radii, m.vdw_radii);
    });
}

int ld_scorer_set_stream(ld_scorer *s, void *hip_stream) {
    return guarded([&] {
        if (!s) throw ld::Error(LD_ERR_INVALID, "null scorer");
        s->impl.set_stream(static_cast<hipStream_t>(hip_stream));
    });
}

int ld_scorer_energy(ld_scorer *s, const double translation[3], const double rotation_wxyz[4], const double *rec_nmodes,
                     const double *lig_nmodes, double *energy_out) {
    return guarded([&] {
        if (!s || !translation || !rotation_wxyz || !energy_out) throw ld::Error(LD_ERR_INVALID, "ld_scorer_energy: null argument");
        ld::Scorer &sc = s->impl;
        std::vector<double> row(sc.pose_len(), 0.0);
        std::memcpy(row.data(), translation, 3 * sizeof(double));
        std::memcpy(row.data() + 3, rotation_wxyz, 4 * sizeof(double));
        if (sc.anm_rec()) {
            if (!rec_nmodes) throw ld::Error(LD_ERR_INVALID, "ld_scorer_energy: rec_nmodes missing");
            std::memcpy(row.data() + 7, rec_nmodes, sc.anm_rec() * sizeof(double));
        }
        if (sc.anm_lig()) {
            if (!lig_nmodes) throw ld::Error(LD_ERR_INVALID, "ld_scorer_energy: lig_nmodes missing");
            std::memcpy(row.data() + 7 + sc.anm_rec(), lig_nmodes, sc.anm_lig() * sizeof(double));
        }
        sc.energy_batch_host(1, row.data(), row.size(), energy_out);
    });
}

int ld_scorer_energy_batch(ld_scorer *s, size_t n, const double *poses, size_t stride, double *energies_out) {
    return guarded([&] {
        if (!s) throw ld::Error(LD_ERR_INVALID, "null scorer");
        s->impl.energy_batch_host(n, poses, stride, energies_out);
    });
}

int ld_scorer_energy_batch_device(ld_scorer *s, size_t n, const double *d_poses, size_t stride, const uint8_t *d_active,
                                  double *d_energies_out, uint32_t *d_pair_counts) {
    return guarded([&] {
        if (!s) throw ld::Error(LD_ERR_INVALID, "null scorer");
        s->impl.energy_batch_device(n, d_poses, stride, d_active, d_energies_out, d_pair_counts);
    });
}

int ld_scorer_last_block_counts(ld_scorer *s, size_t n, uint32_t *blocks_out_host) {
    return guarded([&] {
        if (!s) throw ld::Error(LD_ERR_INVALID, "null scorer");
        s->impl.last_block_counts(n, blocks_out_host);
    });
}

int ld_scorer_bm_quiet_subtiles(const ld_scorer *s, uint32_t *count_out) {
    return guarded([&] {
        if (!s || !count_out) throw ld::Error(LD_ERR_INVALID, "null argument");
        *count_out = s->impl.bm_quiet_subtiles();
    });
}

int ld_scorer_bm_passes(const ld_scorer *s, size_t n, size_t *pass_poses_out, size_t *sets_out) {
    return guarded([&] {
        if (!s) throw ld::Error(LD_ERR_INVALID, "null scorer");
        if (pass_poses_out) *pass_poses_out = s->impl.bm_pass_poses(n);
        if (sets_out) *sets_out = s->impl.bm_sets(n);
    });
}

int ld_scorer_kernel_info(const ld_scorer *s, ld_kernel_info *out) {
    return guarded([&] {
        if (!s || !out) throw ld::Error(LD_ERR_INVALID, "null argument");
        s->impl.kernel_info(out);
    });
}

int ld_scorer_enable_timing(ld_scorer *s, int enable) {
    return guarded([&] {
        if (!s) throw ld::Error(LD_ERR_INVALID, "null scorer");
        s->impl.enable_timing(enable != 0);
    });
}
int ld_scorer_pair_kernel_time(ld_scorer *s, double *total_ms_out, uint64_t *launches_out) {
    return guarded([&] {
        if (!s) throw ld::Error(LD_ERR_INVALID, "null scorer");
        s->impl.pair_kernel_time(total_ms_out, launches_out);
    });
}

int ld_scorer_decompose(ld_scorer *s, size_t n, const double *poses, size_t stride, ld_energy_terms *terms_out,
                        const ld_group_energies *receptor, const ld_group_energies *ligand) {
    return guarded([&] {
        if (!s) throw ld::Error(LD_ERR_INVALID, "null scorer");
        if (n == 0) return;
        s->decompose().run(n, poses, stride, terms_out, receptor, ligand, s->impl.stream());
    });
}
int ld_scorer_decompose_info(const ld_scorer *s, size_t *slice_poses_out, double *last_kernel_ms_out) {
    return guarded([&] {
        if (!s) throw ld::Error(LD_ERR_INVALID, "null scorer");
        if (slice_poses_out) *slice_poses_out = ld::Decomposer::slice_of(s->desc.view());
        if (last_kernel_ms_out) *last_kernel_ms_out = s->decomposer ? s->decomposer->last_kernel_ms() : 0.0;
    });
}

int ld_scorer_refine(ld_scorer *s, const ld_refine_options *opts, size_t n, const double *poses, size_t stride, double *poses_out,
                     ld_refine_stats *stats_out, ld_refine_history *history_out) {
    return guarded([&] {
        if (!s || !opts) throw ld::Error(LD_ERR_INVALID, "null argument");
        s->refine().run(*opts, n, poses, stride, poses_out, stats_out, history_out);
    });
}
int ld_scorer_refine_info(const ld_scorer *s, size_t *trials_out, size_t *slice_poses_out, double *last_kernel_ms_out,
                          uint64_t *evaluations_out) {
    return guarded([&] {
        if (!s) throw ld::Error(LD_ERR_INVALID, "null scorer");
        const ld::RefinePlan plan = ld::refine_plan(s->impl.pose_len(), 0, s->impl.pose_len(), 1, 0);
        if (trials_out) *trials_out = plan.trials;
        if (slice_poses_out) *slice_poses_out = s->refiner && s->refiner->last_slice() ? s->refiner->last_slice() : plan.slice;
        if (last_kernel_ms_out) *last_kernel_ms_out = s->refiner ? s->refiner->last_kernel_ms() : 0.0;
        if (evaluations_out) *evaluations_out = s->refiner ? s->refiner->last_evaluations() : 0;
    });
}
int ld_refine_plan(size_t pose_len, size_t n, size_t stride, uint32_t iterations, uint32_t slice_poses, size_t *trials_out,
                   size_t *slice_poses_out, size_t *workspace_bytes_out) {
    return guarded([&] {
        const ld::RefinePlan plan = ld::refine_plan(pose_len, n, stride, iterations, slice_poses);
        if (trials_out) *trials_out = plan.trials;
        if (slice_poses_out) *slice_poses_out = plan.slice;
        if (workspace_bytes_out) *workspace_bytes_out = plan.workspace_bytes;
    });
}
int ld_refine_trials(size_t n, size_t pose_len, const double *poses, size_t stride, const ld_refine_state *state, double *trials,
                     size_t trial_stride, uint8_t *active_out) {
    return guarded([&] {
        if (!state) throw ld::Error(LD_ERR_INVALID, "null argument");
        ld::refine_trials_host(n, pose_len, poses, stride, *state, trials, trial_stride, active_out);
    });
}
int ld_refine_select(size_t n, size_t pose_len, double *poses, size_t stride, const ld_refine_state *state, const double *energies,
                     uint32_t max_halvings, ld_refine_history *history_out) {
    return guarded([&] {
        if (!state) throw ld::Error(LD_ERR_INVALID, "null argument");
        ld::refine_select_host(n, pose_len, poses, stride, *state, energies, max_halvings, history_out);
    });
}

/* ---- GSO ------------------------------------------------------------------------------ */

ld_gso *ld_gso_create(ld_scorer *scorer, size_t n_swarms, size_t n_glowworms, const double *positions,
                      const uint64_t *seeds) {
    ld_gso *g = nullptr;
    int rc = guarded([&] {
        if (!scorer) throw ld::Error(LD_ERR_INVALID, "ld_gso_create: null scorer");
        g = new ld_gso(scorer->impl, n_swarms, n_glowworms, positions, seeds);
    });
    return rc == LD_OK ? g : nullptr;
}
void ld_gso_destroy(ld_gso *g) { delete g; }

int ld_gso_step(ld_gso *g) {
    return guarded([&] {
        if (!g) throw ld::Error(LD_ERR_INVALID, "null gso");
        g->impl.step();
    });
}
int ld_gso_run(ld_gso *g, uint32_t steps) {
    return guarded([&] {
        if (!g) throw ld::Error(LD_ERR_INVALID, "null gso");
        g->impl.run(steps);
    });
}
uint32_t ld_gso_steps_done(const ld_gso *g) { return g ? g->impl.steps_done() : 0; }
uint64_t ld_gso_num_evals(ld_gso *g) {
    uint64_t n = 0;
    if (g) guarded([&] { n = g->impl.num_evals(); });
    return n;
}
int ld_gso_read(ld_gso *g, size_t swarm, double *poses, double *luciferin, double *vision_range, double *scoring,
                int32_t *n_neighbors, int32_t *moved, int32_t *target) {
    return guarded([&] {
        if (!g) throw ld::Error(LD_ERR_INVALID, "null gso");
        g->impl.read(swarm, poses, luciferin, vision_range, scoring, n_neighbors, moved, target);
    });
}
int ld_gso_save(ld_gso *g, size_t swarm, uint32_t step, const char *dir) {
    return guarded([&] {
        if (!g || !dir) throw ld::Error(LD_ERR_INVALID, "null argument");
        g->impl.save(swarm, step, dir);
    });
}

int ld_gso_save_many(ld_gso *g, size_t n, const size_t *swarms, const char *const *dirs, uint32_t step) {
    return guarded([&] {
        if (!g || (n && (!swarms || !dirs))) throw ld::Error(LD_ERR_INVALID, "null argument");
        std::vector<std::string> d(n);
        for (size_t k = 0; k < n; k++) {
            if (!dirs[k]) throw ld::Error(LD_ERR_INVALID, "null directory");
            d[k] = dirs[k];
        }
        g->impl.save_many(std::vector<size_t>(swarms, swarms + n), step, d);
    });
}

/* ---- the analysis half of a run ---------------------------------------------------------- */

ld_complex *ld_complex_create(const char *receptor_pdb, const char *ligand_pdb, const double *rec_nmodes,
                              size_t rec_nmodes_len, size_t rec_num_anm, const double *lig_nmodes, size_t lig_nmodes_len,
                              size_t lig_num_anm) {
    ld_complex *c = nullptr;
    int rc = guarded([&] {
        c = new ld_complex(receptor_pdb, ligand_pdb, rec_nmodes, rec_nmodes_len, rec_num_anm, lig_nmodes, lig_nmodes_len, lig_num_anm);
    });
    return rc == LD_OK ? c : nullptr;
}
void ld_complex_destroy(ld_complex *c) { delete c; }

size_t ld_complex_pose_len(const ld_complex *c) { return c ? c->impl.pose_len() : 0; }
size_t ld_complex_num_atoms(const ld_complex *c, int side) { return c ? c->impl.num_atoms(side) : 0; }
size_t ld_complex_num_residues(const ld_complex *c, int side) { return c ? c->impl.num_residues(side) : 0; }

int ld_complex_residue_id(const ld_complex *c, int side, size_t index, char *buf, size_t buf_len) {
    return guarded([&] {
        if (!c) throw ld::Error(LD_ERR_INVALID, "null argument");
        c->impl.residue_id(side, index, buf, buf_len);
    });
}
int ld_complex_residue_of_atom(const ld_complex *c, int side, uint32_t *out) {
    return guarded([&] {
        if (!c) throw ld::Error(LD_ERR_INVALID, "null argument");
        c->impl.residue_of_atom(side, out);
    });
}

int ld_complex_coordinates(ld_complex *c, size_t n, const double *poses, size_t stride, double *xyz_out) {
    return guarded([&] {
        if (!c) throw ld::Error(LD_ERR_INVALID, "null argument");
        c->impl.coordinates(n, poses, stride, xyz_out);
    });
}
int ld_complex_cluster(ld_complex *c, size_t n_swarms, size_t n_glowworms, const double *poses, size_t stride,
                       const double *scoring, double cutoff, int32_t *cluster_of, int32_t *representatives,
                       uint32_t *n_clusters) {
    return guarded([&] {
        if (!c) throw ld::Error(LD_ERR_INVALID, "null complex");
        c->impl.cluster(n_swarms, n_glowworms, poses, stride, scoring, cutoff, cluster_of, representatives, n_clusters);
    });
}
int ld_complex_cluster_ranked(ld_complex *c, size_t n, const double *poses, size_t stride, const double *scoring, double cutoff,
                              int atoms, int32_t *cluster_of, int32_t *representatives, uint32_t *n_clusters) {
    return guarded([&] {
        if (!c) throw ld::Error(LD_ERR_INVALID, "null complex");
        c->impl.cluster_ranked(n, poses, stride, scoring, cutoff, atoms, cluster_of, representatives, n_clusters);
    });
}
int ld_complex_contacts(ld_complex *c, size_t n, const double *poses, size_t stride, double cutoff, uint32_t *rec_bits,
                        uint32_t *lig_bits) {
    return guarded([&] {
        if (!c) throw ld::Error(LD_ERR_INVALID, "null complex");
        c->impl.contacts(n, poses, stride, cutoff, rec_bits, lig_bits);
    });
}
int ld_complex_pair_contacts(ld_complex *c, size_t n, const double *poses, size_t stride, double cutoff, uint32_t *offsets, uint32_t *keys,
                             size_t cap, size_t *total_out) {
    return guarded([&] {
        if (!c) throw ld::Error(LD_ERR_INVALID, "null complex");
        c->impl.pair_contacts(n, poses, stride, cutoff, offsets, keys, cap, total_out);
    });
}
int ld_complex_cluster_fcc(ld_complex *c, size_t n, const double *poses, size_t stride, const double *scoring, double cutoff,
                           double threshold, uint32_t min_size, int32_t *cluster_of, int32_t *centres, uint32_t *n_clusters,
                           uint32_t *set_sizes, uint64_t *consensus) {
    return guarded([&] {
        if (!c) throw ld::Error(LD_ERR_INVALID, "null complex");
        c->impl.cluster_fcc(n, poses, stride, scoring, cutoff, threshold, min_size, cluster_of, centres, n_clusters, set_sizes, consensus);
    });
}
int ld_fcc_common(size_t n, const uint32_t *offsets, const uint32_t *keys, uint32_t *common) {
    return guarded([&] { ld::fcc_common_host(n, offsets, keys, common); });
}
int ld_fcc_cluster(size_t n, const uint32_t *offsets, const uint32_t *keys, const double *scoring, double threshold, uint32_t min_size,
                   int32_t *cluster_of, int32_t *centres, uint32_t *n_clusters, uint64_t *consensus) {
    return guarded([&] { ld::fcc_cluster_host(n, offsets, keys, scoring, threshold, min_size, cluster_of, centres, n_clusters, consensus); });
}
int ld_fcc_last_kernel_ms(double *ms_out) {
    return guarded([&] {
        if (!ms_out) throw ld::Error(LD_ERR_INVALID, "null argument");
        *ms_out = ld::fcc_last_kernel_ms();
    });
}
int ld_sasa_directions(int32_t *out) {
    return guarded([&] {
        if (!out) throw ld::Error(LD_ERR_INVALID, "null argument");
        std::memcpy(out, ld::kSasaDirections, sizeof ld::kSasaDirections);
    });
}
int ld_complex_sasa_radii(const ld_complex *c, int side, uint32_t *radii_out) {
    return guarded([&] {
        if (!c) throw ld::Error(LD_ERR_INVALID, "null complex");
        c->impl.sasa_radii(side, radii_out);
    });
}
int ld_complex_sasa(ld_complex *c, size_t n, const double *poses, size_t stride, double probe, uint64_t *sums, uint8_t *free_counts,
                    uint8_t *bound_counts) {
    return guarded([&] {
        if (!c) throw ld::Error(LD_ERR_INVALID, "null complex");
        c->impl.sasa(n, poses, stride, probe, sums, free_counts, bound_counts);
    });
}
int ld_ccs_frames(int32_t *out) {
    return guarded([&] {
        if (!out) throw ld::Error(LD_ERR_INVALID, "null argument");
        std::memcpy(out, ld::kCcsFrames, sizeof ld::kCcsFrames);
    });
}
int ld_complex_ccs(ld_complex *c, size_t n, const double *poses, size_t stride, int what, double probe, double cell, uint32_t *counts,
                   uint64_t *sums) {
    return guarded([&] {
        if (!c) throw ld::Error(LD_ERR_INVALID, "null complex");
        c->impl.ccs(n, poses, stride, what, probe, cell, counts, sums);
    });
}
int ld_complex_crosslinks(ld_complex *c, size_t n, const double *poses, size_t stride, size_t n_links, const uint32_t *links, double probe,
                          double cell, double reach, double max_length, uint64_t *straight2, uint32_t *path) {
    return guarded([&] {
        if (!c) throw ld::Error(LD_ERR_INVALID, "null complex");
        c->impl.crosslinks(n, poses, stride, n_links, links, probe, cell, reach, max_length, straight2, path);
    });
}
int ld_complex_saxs_classes(const ld_complex *c, int side, uint8_t *class_out) {
    return guarded([&] {
        if (!c) throw ld::Error(LD_ERR_INVALID, "null complex");
        c->impl.saxs_classes(side, class_out);
    });
}
int ld_saxs_form_factors(const double *q, size_t n_q, double *f_out) {
    return guarded([&] { ld::saxs_form_factors(q, n_q, f_out); });
}
int ld_saxs_sinc(const double *q, size_t n_q, uint32_t width, size_t bins, double *s_out) {
    return guarded([&] { ld::saxs_sinc(q, n_q, width, bins, s_out); });
}
int ld_complex_distance_histogram(ld_complex *c, size_t n, const double *poses, size_t stride, uint32_t width, size_t bins,
                                  uint32_t *counts) {
    return guarded([&] {
        if (!c) throw ld::Error(LD_ERR_INVALID, "null complex");
        c->impl.distance_histogram(n, poses, stride, width, bins, counts);
    });
}
int ld_saxs_debye(size_t n, const uint32_t *counts, uint32_t width, size_t bins, const uint32_t class_atoms[6], const double *q,
                  size_t n_q, double *intensity) {
    return guarded([&] { ld::saxs_debye_host(n, counts, width, bins, class_atoms, q, n_q, intensity); });
}
int ld_complex_saxs(ld_complex *c, size_t n, const double *poses, size_t stride, uint32_t width, size_t bins, const double *q,
                    size_t n_q, double *intensity, uint32_t *counts) {
    return guarded([&] {
        if (!c) throw ld::Error(LD_ERR_INVALID, "null complex");
        c->impl.saxs(n, poses, stride, width, bins, q, n_q, intensity, counts);
    });
}
int ld_complex_saxs_chunk(ld_complex *c, size_t poses) {
    return guarded([&] {
        if (!c) throw ld::Error(LD_ERR_INVALID, "null complex");
        c->impl.saxs_chunk(poses);
    });
}
int ld_saxs_fit(size_t n, size_t n_q, const double *intensity, const double *i_exp, const double *sigma, double *scale_out,
                double *chi2_out) {
    return guarded([&] { ld::saxs_fit(n, n_q, intensity, i_exp, sigma, scale_out, chi2_out); });
}
ld_density *ld_density_create(const float *rho, const uint32_t n[3], const int32_t origin[3], const uint32_t step[3], double threshold) {
    ld_density *d = nullptr;
    int rc = guarded([&] { d = new ld_density(rho, n, origin, step, threshold); });
    return rc == LD_OK ? d : nullptr;
}
void ld_density_destroy(ld_density *d) { delete d; }
int ld_density_info(const ld_density *d, uint64_t *n_voxels, uint64_t *s_e, uint64_t *s_ee, double *scale) {
    return guarded([&] {
        if (!d) throw ld::Error(LD_ERR_INVALID, "null density");
        if (n_voxels) *n_voxels = d->impl.voxels();
        if (s_e) *s_e = d->impl.s_e();
        if (s_ee) *s_ee = d->impl.s_ee();
        if (scale) *scale = d->impl.scale();
    });
}
int ld_density_voxels(const ld_density *d, uint32_t *voxels_out) {
    return guarded([&] {
        if (!d || !voxels_out) throw ld::Error(LD_ERR_INVALID, "null argument");
        const std::vector<uint16_t> &E = d->impl.E();
        for (size_t v = 0; v < E.size(); v++) voxels_out[v] = E[v];
    });
}
int ld_density_kernel(uint32_t sigma, uint32_t *table_out, uint32_t *length_out, uint32_t *shift_out) {
    return guarded([&] {
        const ld::DensityKernel k = ld::density_kernel(sigma);
        if (table_out) std::copy(k.table.begin(), k.table.end(), table_out);
        if (length_out) *length_out = (uint32_t)k.table.size();
        if (shift_out) *shift_out = k.shift;
    });
}
int ld_complex_density_fit(ld_complex *c, ld_density *d, size_t n, const double *poses, size_t stride, uint32_t sigma, ld_density_sums *out) {
    return guarded([&] {
        if (!c || !d) throw ld::Error(LD_ERR_INVALID, "null argument");
        c->impl.density_fit(d->impl, n, poses, stride, sigma, out);
    });
}
int ld_complex_simulate_density(ld_complex *c, ld_density *d, size_t n, const double *poses, size_t stride, uint32_t sigma, uint32_t *grid) {
    return guarded([&] {
        if (!c || !d) throw ld::Error(LD_ERR_INVALID, "null argument");
        c->impl.simulate_density(d->impl, n, poses, stride, sigma, grid);
    });
}
int ld_density_scores(const ld_density *d, size_t n, const ld_density_sums *sums, double *cc, double *ccm, double *inside) {
    return guarded([&] {
        if (!d) throw ld::Error(LD_ERR_INVALID, "null density");
        d->impl.scores(n, sums, cc, ccm, inside);
    });
}
int ld_complex_density_chunk(ld_complex *c, size_t poses) {
    return guarded([&] {
        if (!c) throw ld::Error(LD_ERR_INVALID, "null complex");
        c->impl.density_chunk(poses);
    });
}
int ld_complex_set_reference(ld_complex *c, const char *ref_receptor_pdb, const char *ref_ligand_pdb, double contact_cutoff,
                             double interface_cutoff) {
    return guarded([&] {
        if (!c) throw ld::Error(LD_ERR_INVALID, "null complex");
        c->impl.set_reference(ref_receptor_pdb, ref_ligand_pdb, contact_cutoff, interface_cutoff);
    });
}
int ld_complex_reference_counts(const ld_complex *c, uint32_t *out) {
    return guarded([&] {
        if (!c) throw ld::Error(LD_ERR_INVALID, "null complex");
        c->impl.reference_counts(out);
    });
}
int ld_complex_native_pairs(const ld_complex *c, uint32_t *pairs) {
    return guarded([&] {
        if (!c) throw ld::Error(LD_ERR_INVALID, "null complex");
        c->impl.native_pairs(pairs);
    });
}
int ld_complex_assess(ld_complex *c, size_t n, const double *poses, size_t stride, uint32_t *kept, double *lrmsd, double *irmsd) {
    return guarded([&] {
        if (!c) throw ld::Error(LD_ERR_INVALID, "null complex");
        c->impl.assess(n, poses, stride, kept, lrmsd, irmsd);
    });
}
int ld_complex_last_kernel_ms(const ld_complex *c, double *ms_out) {
    return guarded([&] {
        if (!c || !ms_out) throw ld::Error(LD_ERR_INVALID, "null argument");
        *ms_out = c->impl.last_kernel_ms();
    });
}
int ld_complex_write_pdb(ld_complex *c, const double *pose, const char *path) {
    return guarded([&] {
        if (!c) throw ld::Error(LD_ERR_INVALID, "null argument");
        c->impl.write_pdb(pose, path);
    });
}

int ld_anm_nodes(const char *pdb_path, uint32_t *node_atom_out, size_t *n_residues_out) {
    return guarded([&] {
        if (!pdb_path || !n_residues_out) throw ld::Error(LD_ERR_INVALID, "null argument");
        const std::vector<uint32_t> node = ld::anm_node_atoms(ld::read_pdb_file_order(pdb_path));
        *n_residues_out = node.size();
        if (node_atom_out) std::memcpy(node_atom_out, node.data(), node.size() * sizeof(uint32_t));
    });
}
int ld_anm_modes_xyz(const double *node_xyz, size_t n_nodes, size_t n_modes, double cutoff, double *node_modes_out,
                     double *eigenvalues_out) {
    return guarded([&] {
        if (!node_xyz || !node_modes_out) throw ld::Error(LD_ERR_INVALID, "null argument");
        const ld::AnmResult r = ld::anm_solve(node_xyz, n_nodes, n_modes, cutoff, nullptr, n_nodes, 0.0);
        std::memcpy(node_modes_out, r.modes.data(), r.modes.size() * sizeof(double));
        if (eigenvalues_out) std::memcpy(eigenvalues_out, r.eigenvalues.data(), r.eigenvalues.size() * sizeof(double));
    });
}
int ld_anm_modes(const char *pdb_path, size_t n_modes, double cutoff, double rmsd, double *modes_out, double *eigenvalues_out) {
    return guarded([&] {
        if (!pdb_path || !modes_out) throw ld::Error(LD_ERR_INVALID, "null argument");
        const ld::PdbFile pdb = ld::read_pdb_file_order(pdb_path);
        const std::vector<uint32_t> node = ld::anm_node_atoms(pdb);
        std::vector<double> xyz(3 * node.size());
        for (size_t r = 0; r < node.size(); r++)
            for (int c = 0; c < 3; c++) xyz[3 * r + c] = pdb.xyz[3 * (size_t)node[r] + c];
        const ld::AnmResult r = ld::anm_solve(xyz.data(), node.size(), n_modes, cutoff, pdb.res_of_atom.data(), pdb.res_of_atom.size(), rmsd);
        std::memcpy(modes_out, r.modes.data(), r.modes.size() * sizeof(double));
        if (eigenvalues_out) std::memcpy(eigenvalues_out, r.eigenvalues.data(), r.eigenvalues.size() * sizeof(double));
    });
}
int ld_anm_last_kernel_ms(double *ms_out) {
    return guarded([&] {
        if (!ms_out) throw ld::Error(LD_ERR_INVALID, "null argument");
        *ms_out = ld::anm_last_kernel_ms();
    });
}

int ld_swarm_diameter2(const int32_t *xyz, size_t n, uint64_t *d2_out) {
    return guarded([&] {
        if (!xyz || !d2_out) throw ld::Error(LD_ERR_INVALID, "null argument");
        *d2_out = ld::swarm_diameter2(xyz, n);
    });
}
int ld_swarm_shell(const int32_t *atoms, const uint8_t *bead, size_t n, int32_t spacing, int32_t *nodes_out, size_t cap,
                   size_t *count_out, uint64_t *lattice_nodes_out) {
    return guarded([&] {
        if (!atoms || !count_out) throw ld::Error(LD_ERR_INVALID, "null argument");
        const ld::SwarmShell shell = ld::swarm_shell(atoms, bead, n, spacing);
        const size_t count = shell.candidates.size() / 3;
        *count_out = count;
        if (nodes_out && cap < count)
            throw ld::Error(LD_ERR_INVALID, "room for " + std::to_string(cap) + " candidates, the shell has " + std::to_string(count));
        if (lattice_nodes_out) *lattice_nodes_out = shell.nodes;
        if (nodes_out && count) std::memcpy(nodes_out, shell.candidates.data(), shell.candidates.size() * sizeof(int32_t));
    });
}
int ld_swarm_centres(const int32_t *points, size_t n, size_t max_centres, int32_t cover, uint32_t *index_out, uint64_t *gap2_out,
                     size_t *n_out) {
    return guarded([&] {
        if ((!points && n) || !index_out || !gap2_out || !n_out) throw ld::Error(LD_ERR_INVALID, "null argument");
        const ld::SwarmCentres c = ld::swarm_centres(points, n, max_centres, cover);
        if (!c.index.empty()) {
            std::memcpy(index_out, c.index.data(), c.index.size() * sizeof(uint32_t));
            std::memcpy(gap2_out, c.gap2.data(), c.gap2.size() * sizeof(uint64_t));
        }
        *n_out = c.index.size();
    });
}
int ld_initial_poses(uint64_t seed, size_t glowworms, size_t swarm, size_t first, size_t n, const double centre[3], double radius,
                     const double *rec_points, size_t n_rec, const double *lig_points, size_t n_lig, size_t anm_rec, size_t anm_lig,
                     double *rows_out, uint64_t *draws_out) {
    return guarded([&] {
        if (!centre || (n && !rows_out)) throw ld::Error(LD_ERR_INVALID, "null argument");
        ld::PoseRequest r;
        r.seed = seed;
        r.glowworms = glowworms;
        r.swarm = swarm;
        r.first = first;
        r.n = n;
        std::memcpy(r.centre, centre, sizeof r.centre);
        r.radius = radius;
        r.rec_points = rec_points;
        r.n_rec = n_rec;
        r.lig_points = lig_points;
        r.n_lig = n_lig;
        r.anm_rec = anm_rec;
        r.anm_lig = anm_lig;
        ld::initial_poses(r, rows_out, draws_out);
    });
}
int ld_prepare_pdb(const char *in_path, const char *out_path, int keep_flags, size_t *atoms_out, double centre_out[3]) {
    return guarded([&] {
        const ld::PreparedPdb p = ld::prepare_pdb(in_path, out_path, keep_flags);
        if (atoms_out) *atoms_out = p.atoms;
        if (centre_out) std::memcpy(centre_out, p.centre, sizeof p.centre);
    });
}
int ld_setup_last_kernel_ms(double *ms_out) {
    return guarded([&] {
        if (!ms_out) throw ld::Error(LD_ERR_INVALID, "null argument");
        *ms_out = ld::setup_last_kernel_ms();
    });
}

int ld_cli_main(int argc, char **argv) {
    int code = 0;
    int rc = guarded([&] { code = ld::cli_main(argc, argv); });
    if (rc != LD_OK) {
        std::fprintf(stderr, "%s\n", g_last_error.c_str());
        return 101;  // the reference's panic exit code
    }
    return code;
}

}  // extern "C"
