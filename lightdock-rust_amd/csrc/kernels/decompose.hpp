// decompose.hpp -- launch interface of the energy-decomposition kernels (K1d; include/lightdock_hip.h "Energy decomposition").
//
// Three steps per pass of poses, all in the reference's atom order and with a defined order of every sum:
//   decompose_pose    each pose's ligand (with receptor ANM also its receptor) as f64 SoA into the per-pose workspace;
//   decompose_side    one 256-thread workgroup per (pose, 256 owner atoms): a lane owns one atom, keeps its accumulators in
//                     registers and walks the partner molecule through LDS in ascending index; launched once with the
//                     receptor owning and once with the ligand owning;
//   decompose_groups  one thread per (pose, group) over a CSR of the group's atoms, ascending;
//   decompose_terms   one thread per pose: ld_energy_terms from the receptor atoms' sums and both sides' flags.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "lightdock_hip.h"

namespace ld {

constexpr int kDecomposeThreads = 256;                           // owner atoms per workgroup, 4 wave64
constexpr int kDecomposeChunk = 512;                               // partner records per LDS chunk: 16 KiB (DFIRE) / 32 KiB (DNA)
constexpr size_t kDecomposeWorkspaceBytes = (size_t)64 << 20;    // bound of a pass's per-pose workspace
constexpr size_t kDecomposeMaxSlice = 4096;                      // poses per pass at most

// One molecule on the device in the reference's atom order, SoA, every array n_pad long (a multiple of 64).
struct DecomposeMolecule {
    int n = 0, n_pad = 0;
    const double *x = nullptr, *y = nullptr, *z = nullptr;
    const uint32_t *tindex = nullptr;   // DFIRE: receptor type * 3380, ligand type * 20
    const double *charge = nullptr, *eps = nullptr, *radius = nullptr;   // DNA: as the model has them (eps is NOT a root)
    int num_anm = 0;                    // modes a pose carries for this side: 0 unless the scorer uses ANM
    const double *modes = nullptr;      // [mode][xyz][n_pad]
};

// Per-pose bytes of the workspace below.
inline size_t decompose_pose_bytes(int rec_n_pad, int lig_n_pad, bool rec_flexes) {
    const size_t atoms = (size_t)rec_n_pad + (size_t)lig_n_pad;
    return 24 * (size_t)lig_n_pad + (rec_flexes ? 24 * (size_t)rec_n_pad : 0) + atoms * (16 + 4 + 4);
}
inline size_t decompose_slice(int rec_n_pad, int lig_n_pad, bool rec_flexes) {
    const size_t s = kDecomposeWorkspaceBytes / decompose_pose_bytes(rec_n_pad, lig_n_pad, rec_flexes);
    return s < 1 ? 1 : s > kDecomposeMaxSlice ? kDecomposeMaxSlice : s;
}

struct DecomposeLaunch {
    int method = 0;   // 0 DFIRE, 1 DNA / PYDOCK
    DecomposeMolecule rec, lig;
    const double *table = nullptr;      // DFIRE: the potential in the reference's layout (LD_DFIRE_TABLE_LEN)
    const uint8_t *lut = nullptr;       // DFIRE: kDfireLutCells
    const double *bin_step = nullptr;   // DFIRE: kDfireSteps
    double iface_d2 = 0.0;              // a pair is interface iff d2 <= iface_d2
    // the pass
    const double *poses = nullptr;      // device, row p at poses + p * stride
    size_t stride = 0;
    int n_poses = 0;
    // workspace, [pose] outermost
    double *lig_xyz = nullptr;          // [pose][3][lig.n_pad]
    double *rec_xyz = nullptr;          // [pose][3][rec.n_pad]; null: the receptor does not flex, rec.x/y/z are read
    double *rec_sum = nullptr, *lig_sum = nullptr;           // [pose][2][n_pad]
    uint32_t *rec_pairs = nullptr, *lig_pairs = nullptr;     // [pose][n_pad]
    uint32_t *rec_flag = nullptr, *lig_flag = nullptr;       // [pose][n_pad], 0 / 1
};

// The groups of one side as a CSR in ascending atom order, and where a pass's rows go (device; any output may be null).
struct DecomposeGroups {
    int n_groups = 0;
    const uint32_t *offsets = nullptr;   // n_groups + 1
    const uint32_t *atoms = nullptr;
    double *sums = nullptr;              // [pose][group][2]
    uint32_t *pairs = nullptr, *iface = nullptr;   // [pose][group]
};

// src/scoring.rs:21-47 over atom indices: the restraint groups of both sides and the receptor's beads.
struct DecomposeTail {
    int n_rec_groups = 0, n_lig_groups = 0, n_membrane = 0;
    const uint32_t *rec_offsets = nullptr, *rec_atoms = nullptr;
    const uint32_t *lig_offsets = nullptr, *lig_atoms = nullptr;
    const uint32_t *membrane = nullptr;
};

hipError_t launch_decompose_pose(const DecomposeLaunch &d, hipStream_t stream);
hipError_t launch_decompose_side(const DecomposeLaunch &d, int side /* the owner: 0 receptor, 1 ligand */, hipStream_t stream);
hipError_t launch_decompose_groups(const DecomposeLaunch &d, int side, const DecomposeGroups &g, hipStream_t stream);
hipError_t launch_decompose_terms(const DecomposeLaunch &d, const DecomposeTail &t, ld_energy_terms *terms /* [pose], device */, hipStream_t stream);

}  // namespace ld
