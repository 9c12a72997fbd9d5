// decompose.hip -- K1d: the energy decomposition for gfx950 (MI355X); interface and overview in decompose.hpp, the
// definition in include/lightdock_hip.h "Energy decomposition", the arithmetic of a pose and a pair in decompose_pair.hpp.
//
// decompose_side is pose_energy_pairs (pose_energy.hip) turned round: there a lane's pairs are folded in a tree and a pose's
// sum has no order; here a lane OWNS an atom, keeps that atom's accumulators in registers and walks the whole partner molecule
// alone, chunk after chunk through LDS, every lane reading the same record (a broadcast) in ascending index -- which IS the
// sequential sum of the definition.  No atomics, no cross-lane reduction: nothing depends on the launch shape.  Every pair is
// evaluated twice, once per owning side.  Compiled with -ffp-contract=off; no reciprocal approximations, no fmin / fmax.
#include "decompose.hpp"

#include <type_traits>

#include "decompose_pair.hpp"
#include "pose_energy.hpp"

namespace ld {

namespace {

using namespace decompose;

struct alignas(16) DfireRec {
    double x, y, z;
    uint32_t tindex;
    uint32_t pad;
};
static_assert(sizeof(DfireRec) == 32, "DfireRec must be 32 bytes");

struct alignas(16) DnaRec {
    double x, y, z;
    double charge, eps, radius;
    double pad[2];
};
static_assert(sizeof(DnaRec) == 64, "DnaRec must be 64 bytes");

constexpr size_t kLutBytes = (kDfireLutCells + 15) & ~15;

// One thread per (pose, atom): the ligand's atoms first, then (a receptor that flexes) the receptor's.
__global__ __launch_bounds__(kDecomposeThreads) void decompose_pose(const DecomposeLaunch D) {
    const size_t per_pose = (size_t)D.lig.n + (D.rec_xyz ? (size_t)D.rec.n : 0);
    const size_t t = (size_t)blockIdx.x * kDecomposeThreads + threadIdx.x;
    if (t >= per_pose * (size_t)D.n_poses) return;
    const size_t pose = t / per_pose;
    size_t atom = t % per_pose;
    const bool ligand = atom < (size_t)D.lig.n;
    if (!ligand) atom -= (size_t)D.lig.n;
    const DecomposeMolecule &m = ligand ? D.lig : D.rec;
    const double *row = D.poses + pose * D.stride;
    const double *ext = row + 7 + (ligand ? D.rec.num_anm : 0);
    double v[3];
    pose_atom(ligand, row, m.x[atom], m.y[atom], m.z[atom], m.num_anm, m.modes, (size_t)m.n_pad, atom, ext, v);
    double *out = (ligand ? D.lig_xyz : D.rec_xyz) + pose * 3 * (size_t)m.n_pad;
    out[atom] = v[0];
    out[(size_t)m.n_pad + atom] = v[1];
    out[2 * (size_t)m.n_pad + atom] = v[2];
}

template <int METHOD, int SIDE>
__global__ __launch_bounds__(kDecomposeThreads) void decompose_side(const DecomposeLaunch D) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using Rec = typename std::conditional<METHOD == 0, DfireRec, DnaRec>::type;
    Rec *rec = reinterpret_cast<Rec *>(smem);
    uint8_t *lut = smem + (size_t)kDecomposeChunk * sizeof(Rec);                                         // DFIRE only
    double *bin_step = reinterpret_cast<double *>(smem + (size_t)kDecomposeChunk * sizeof(Rec) + kLutBytes);   // DFIRE only

    const DecomposeMolecule &own = SIDE == 0 ? D.rec : D.lig;
    const DecomposeMolecule &oth = SIDE == 0 ? D.lig : D.rec;
    const int tid = threadIdx.x;
    const unsigned blocks_per_pose = (unsigned)((own.n + kDecomposeThreads - 1) / kDecomposeThreads);
    const size_t pose = blockIdx.x / blocks_per_pose;
    const int atom = (int)(blockIdx.x % blocks_per_pose) * kDecomposeThreads + tid;
    const bool valid = atom < own.n;

    // both molecules as posed: the ligand's from the workspace, the receptor's too where it flexes
    const double *rx = D.rec_xyz ? D.rec_xyz + pose * 3 * (size_t)D.rec.n_pad : D.rec.x;
    const double *ry = D.rec_xyz ? rx + D.rec.n_pad : D.rec.y;
    const double *rz = D.rec_xyz ? ry + D.rec.n_pad : D.rec.z;
    const double *lx = D.lig_xyz + pose * 3 * (size_t)D.lig.n_pad;
    const double *ly = lx + D.lig.n_pad, *lz = ly + D.lig.n_pad;
    const double *ox = SIDE == 0 ? rx : lx, *oy = SIDE == 0 ? ry : ly, *oz = SIDE == 0 ? rz : lz;
    const double *px = SIDE == 0 ? lx : rx, *py = SIDE == 0 ? ly : ry, *pz = SIDE == 0 ? lz : rz;

    const int a = valid ? atom : 0;
    const double mx = valid ? ox[a] : 1.0e30, my = oy[a], mz = oz[a];   // a padded lane sits outside every cutoff
    uint32_t my_t = 0;
    double my_q = 0.0, my_e = 0.0, my_r = 0.0;
    if constexpr (METHOD == 0) {
        my_t = own.tindex[a];
    } else {
        my_q = own.charge[a];
        my_e = own.eps[a];
        my_r = own.radius[a];
    }
    if constexpr (METHOD == 0) {
        for (int i = tid; i < kDfireLutCells / 4; i += kDecomposeThreads)
            reinterpret_cast<uint32_t *>(lut)[i] = reinterpret_cast<const uint32_t *>(D.lut)[i];
        if (tid < kDfireSteps) bin_step[tid] = D.bin_step[tid];
    }

    double acc0 = 0.0, acc1 = 0.0;   // DFIRE: the table sum | DNA: electrostatics, van der Waals
    uint32_t cnt = 0, flag = 0;
    for (int c0 = 0; c0 < oth.n; c0 += kDecomposeChunk) {
        const int cn = min(kDecomposeChunk, oth.n - c0);
        __syncthreads();   // the chunk before this one has been walked by every lane
        for (int i = tid; i < cn; i += kDecomposeThreads) {
            Rec r;
            r.x = px[c0 + i];
            r.y = py[c0 + i];
            r.z = pz[c0 + i];
            if constexpr (METHOD == 0) {
                r.tindex = oth.tindex[c0 + i];
                r.pad = 0;
            } else {
                r.charge = oth.charge[c0 + i];
                r.eps = oth.eps[c0 + i];
                r.radius = oth.radius[c0 + i];
                r.pad[0] = r.pad[1] = 0.0;
            }
            rec[i] = r;
        }
        __syncthreads();
        for (int j = 0; j < cn; j++) {
            const Rec p = rec[j];
            const double d2 = SIDE == 0 ? dist2(mx, my, mz, p.x, p.y, p.z) : dist2(p.x, p.y, p.z, mx, my, mz);
            if constexpr (METHOD == 0) {
                if (d2 <= 225.0) {   // src/dfire.rs:334-343
                    acc0 += D.table[my_t + p.tindex + dfire_bin(d2, lut, bin_step)];
                    cnt++;
                    if (d2 <= D.iface_d2) flag = 1;
                }
            } else {
                if (d2 <= kElecCutoff2) {
                    acc0 += SIDE == 0 ? dna_elec(my_q, p.charge, d2) : dna_elec(p.charge, my_q, d2);
                    cnt++;
                }
                if (d2 <= kVdwCutoff2)
                    acc1 += SIDE == 0 ? dna_vdw(my_e, p.eps, my_r, p.radius, d2) : dna_vdw(p.eps, my_e, p.radius, my_r, d2);
                if (d2 <= D.iface_d2) flag = 1;
            }
        }
    }
    if (!valid) return;
    double *sum = (SIDE == 0 ? D.rec_sum : D.lig_sum) + pose * 2 * (size_t)own.n_pad;
    sum[atom] = acc0;
    sum[(size_t)own.n_pad + atom] = acc1;
    (SIDE == 0 ? D.rec_pairs : D.lig_pairs)[pose * (size_t)own.n_pad + atom] = cnt;
    (SIDE == 0 ? D.rec_flag : D.lig_flag)[pose * (size_t)own.n_pad + atom] = flag;
}

// One thread per (pose, group): the group's atoms in ascending index.
__global__ __launch_bounds__(kDecomposeThreads) void decompose_groups(const DecomposeLaunch D, const int side, const DecomposeGroups G) {
    const size_t t = (size_t)blockIdx.x * kDecomposeThreads + threadIdx.x;
    if (t >= (size_t)D.n_poses * (size_t)G.n_groups) return;
    const size_t pose = t / (size_t)G.n_groups;
    const size_t g = t % (size_t)G.n_groups;
    const size_t n_pad = (size_t)(side == 0 ? D.rec.n_pad : D.lig.n_pad);
    const double *sum = (side == 0 ? D.rec_sum : D.lig_sum) + pose * 2 * n_pad;
    const uint32_t *pairs = (side == 0 ? D.rec_pairs : D.lig_pairs) + pose * n_pad;
    const uint32_t *flag = (side == 0 ? D.rec_flag : D.lig_flag) + pose * n_pad;
    double s0 = 0.0, s1 = 0.0;
    uint32_t cnt = 0, iface = 0;
    for (uint32_t k = G.offsets[g]; k < G.offsets[g + 1]; k++) {
        const uint32_t a = G.atoms[k];
        s0 += sum[a];
        s1 += sum[n_pad + a];
        cnt += pairs[a];
        iface += flag[a];
    }
    if (G.sums) {
        G.sums[2 * t] = s0;
        G.sums[2 * t + 1] = s1;
    }
    if (G.pairs) G.pairs[t] = cnt;
    if (G.iface) G.iface[t] = iface;
}

// scoring.rs:21-36 over per-atom flags
__device__ double satisfied_fraction(const uint32_t *flag, int n_groups, const uint32_t *offsets, const uint32_t *atoms) {
    if (n_groups == 0) return 0.0;
    int hit = 0;
    for (int g = 0; g < n_groups; g++)
        for (uint32_t k = offsets[g]; k < offsets[g + 1]; k++)
            if (flag[atoms[k]]) {
                hit++;
                break;
            }
    return (double)hit / (double)n_groups;
}

// One thread per pose.
__global__ __launch_bounds__(kDecomposeThreads) void decompose_terms(const DecomposeLaunch D, const DecomposeTail T, ld_energy_terms *terms) {
    const size_t pose = (size_t)blockIdx.x * kDecomposeThreads + threadIdx.x;
    if (pose >= (size_t)D.n_poses) return;
    const size_t nr_pad = (size_t)D.rec.n_pad, nl_pad = (size_t)D.lig.n_pad;
    const double *sum = D.rec_sum + pose * 2 * nr_pad;
    const uint32_t *pairs = D.rec_pairs + pose * nr_pad;
    const uint32_t *rflag = D.rec_flag + pose * nr_pad, *lflag = D.lig_flag + pose * nl_pad;
    double s0 = 0.0, s1 = 0.0;
    uint32_t cnt = 0, ri = 0, li = 0;
    for (int a = 0; a < D.rec.n; a++) {
        s0 += sum[a];
        s1 += sum[nr_pad + a];
        cnt += pairs[a];
        ri += rflag[a];
    }
    for (int a = 0; a < D.lig.n; a++) li += lflag[a];
    double score;
    if (D.method == 0) {
        score = (s0 * 0.0157 - 4.7) * -1.0;   // src/dfire.rs:347
    } else {
        const double total_elec = s0 * 332.0 / 4.0;   // src/dna.rs:513
        score = (total_elec + s1) * -1.0;             // src/dna.rs:514
    }
    const double pr = satisfied_fraction(rflag, T.n_rec_groups, T.rec_offsets, T.rec_atoms);
    const double pl = satisfied_fraction(lflag, T.n_lig_groups, T.lig_offsets, T.lig_atoms);
    double intersection = 0.0, penalty = 0.0;
    if (T.n_membrane > 0) {   // src/scoring.rs:38-47, src/dfire.rs:355-359
        uint32_t beads = 0;
        for (int k = 0; k < T.n_membrane; k++) beads += rflag[T.membrane[k]];
        intersection = (double)beads / (double)T.n_membrane;
        if (intersection > 0.0) penalty = 999.0 * intersection;
    }
    ld_energy_terms out;
    out.pair[0] = s0;
    out.pair[1] = s1;
    out.score = score;
    out.rec_restraints = pr;
    out.lig_restraints = pl;
    out.membrane = intersection;
    out.energy = score + pr * score + pl * score - penalty;   // src/dfire.rs:361
    out.pairs = cnt;
    out.rec_interface = ri;
    out.lig_interface = li;
    out.reserved = 0;
    terms[pose] = out;
}

size_t side_lds_bytes(int method) {
    return method == 0 ? (size_t)kDecomposeChunk * sizeof(DfireRec) + kLutBytes + kDfireSteps * sizeof(double)
                       : (size_t)kDecomposeChunk * sizeof(DnaRec);
}

bool grid_of(size_t threads, dim3 *grid) {
    const size_t blocks = (threads + kDecomposeThreads - 1) / kDecomposeThreads;
    if (blocks == 0 || blocks > 0x7fffffffULL) return false;
    *grid = dim3((unsigned)blocks);
    return true;
}

}  // namespace

hipError_t launch_decompose_pose(const DecomposeLaunch &d, hipStream_t stream) {
    if (d.n_poses <= 0) return hipSuccess;
    dim3 grid;
    if (!grid_of((size_t)d.n_poses * ((size_t)d.lig.n + (d.rec_xyz ? (size_t)d.rec.n : 0)), &grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(decompose_pose, grid, dim3(kDecomposeThreads), 0, stream, d);
    return hipGetLastError();
}

hipError_t launch_decompose_side(const DecomposeLaunch &d, int side, hipStream_t stream) {
    if (d.n_poses <= 0) return hipSuccess;
    const int own = side == 0 ? d.rec.n : d.lig.n;
    const size_t blocks = (size_t)d.n_poses * (size_t)((own + kDecomposeThreads - 1) / kDecomposeThreads);
    if (blocks == 0 || blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(kDecomposeThreads);
    const size_t lds = side_lds_bytes(d.method);
    if (d.method == 0) {
        if (side == 0) hipLaunchKernelGGL((decompose_side<0, 0>), grid, block, lds, stream, d);
        else hipLaunchKernelGGL((decompose_side<0, 1>), grid, block, lds, stream, d);
    } else {
        if (side == 0) hipLaunchKernelGGL((decompose_side<1, 0>), grid, block, lds, stream, d);
        else hipLaunchKernelGGL((decompose_side<1, 1>), grid, block, lds, stream, d);
    }
    return hipGetLastError();
}

hipError_t launch_decompose_groups(const DecomposeLaunch &d, int side, const DecomposeGroups &g, hipStream_t stream) {
    if (d.n_poses <= 0 || g.n_groups <= 0) return hipSuccess;
    dim3 grid;
    if (!grid_of((size_t)d.n_poses * (size_t)g.n_groups, &grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(decompose_groups, grid, dim3(kDecomposeThreads), 0, stream, d, side, g);
    return hipGetLastError();
}

hipError_t launch_decompose_terms(const DecomposeLaunch &d, const DecomposeTail &t, ld_energy_terms *terms, hipStream_t stream) {
    if (d.n_poses <= 0) return hipSuccess;
    dim3 grid;
    if (!grid_of((size_t)d.n_poses, &grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(decompose_terms, grid, dim3(kDecomposeThreads), 0, stream, d, t, terms);
    return hipGetLastError();
}

}  // namespace ld
