// dfire_tiled.hip -- the receptor image of the culled DFIRE kernels (gfx950 / MI355X): pair records in the
// f32 frame of dfire_packed.hpp plus the boxes of every 8-atom subtile and 64-atom tile, in the tile order
// of dfire_tiled.hpp.  The pose-major kernel (dfire_packed.hip) and the block-major path (dfire_bm.hip)
// both read it: once per scorer for a rigid receptor, one image per pose with receptor ANM.
// Compiled with -ffp-contract=off.
#include "dfire_tiled.hpp"

#include <cmath>

#include "dfire_device.hpp"
#include "dfire_packed.hpp"

namespace ld {

namespace {

// ---------------------------------------------------------------------------------------------
// Receptor image: one wave per (receptor tile, 16 poses); lane = atom, the tile's modes stay in registers.
// ---------------------------------------------------------------------------------------------
constexpr int kPreparePoses = 16;   // poses per workgroup: the tile's modes are read once for all of them
constexpr int kPrepareModes = 10;   // modes kept in registers; any further ones are read per pose
__global__ __launch_bounds__(64) void dfire_packed_prepare(const PackedPrepareLaunch P) {
    const int tile = blockIdx.x % (unsigned)P.n_tiles;
    const size_t pose0 = (size_t)(blockIdx.x / (unsigned)P.n_tiles) * kPreparePoses;
    const int lane = threadIdx.x;
    const int a = tile * 64 + lane;
    const size_t pad = (size_t)P.n_tiles * 64;
    const double x0 = P.x[a], y0 = P.y[a], z0 = P.z[a];
    double mx[kPrepareModes], my[kPrepareModes], mz[kPrepareModes];
#pragma unroll
    for (int k = 0; k < kPrepareModes; k++) {
        const bool have = k < P.num_anm;
        const double *m = P.modes + (size_t)(have ? k : 0) * 3 * pad;
        mx[k] = have ? m[a] : 0.0;
        my[k] = have ? m[pad + a] : 0.0;
        mz[k] = have ? m[2 * pad + a] : 0.0;
    }
    const bool real = a < P.n_real;  // padding sits at x = -1e30 (scorer.cpp)
    const uint32_t my_term = P.tindex[a];
    const unsigned long long tracked = __ballot(real && P.slot[a] >= 0);  // atoms with an interface-flag slot
    for (int i = 0; i < kPreparePoses; i++) {
    const size_t pose = pose0 + i;
    if (pose >= P.n_poses) break;
    if (P.active != nullptr && P.active[pose] == 0) continue;
    double x = x0, y = y0, z = z0;
    if (P.num_anm > 0) {  // src/dfire.rs:304-320
        const double *rec_nm = P.poses + pose * P.stride + 7;
#pragma unroll
        for (int k = 0; k < kPrepareModes; k++) {
            if (k < P.num_anm) {
                const double c = rec_nm[k];
                x += mx[k] * c;
                y += my[k] * c;
                z += mz[k] * c;
            }
        }
        for (int k = kPrepareModes; k < P.num_anm; k++) {
            const double c = rec_nm[k];
            const double *m = P.modes + (size_t)k * 3 * pad;
            x += m[a] * c;
            y += m[pad + a] * c;
            z += m[2 * pad + a] * c;
        }
    }
    const float fx = frame_coord(x, P.cx, P.kappa), fy = frame_coord(y, P.cy, P.kappa), fz = frame_coord(z, P.cz, P.kappa);
    const bool inside = fabsf(fx) <= P.ubound && fabsf(fy) <= P.ubound && fabsf(fz) <= P.ubound;
    // record (4 j + q) of the tile holds the atoms (2 q, 2 q + 1) of its subtile j
    float *rec = reinterpret_cast<float *>(P.pairs_out + (pose * (size_t)P.n_tiles + tile) * 32 + (lane >> 1));
    const int h = lane & 1;
    rec[h] = real ? fx : -1.0e30f;
    rec[2 + h] = real ? fy : 0.f;
    rec[4 + h] = real ? fz : 0.f;
    reinterpret_cast<uint32_t *>(rec)[6 + h] = my_term | (real && !inside ? kPackedSlow : 0u);
    BoxRegs b = lane_box(real, fx, fy, fz);
    box_reduce8(b);
    {
        BoxRegs sub = b;
        box_widen(sub);
        if ((lane & 7) == 0) P.sub_out[(pose * (size_t)P.n_tiles + tile) * 8 + (lane >> 3)] = to_box(sub);
    }
    box_reduce64_from8(b);
    box_widen(b);
    // atoms with an interface-flag slot (restraint atoms, membrane beads): one bit per atom of the tile
    if (lane == 63) {
        TiledBox t = to_box(b);
        t.pad0 = __uint_as_float((uint32_t)tracked);
        t.pad1 = __uint_as_float((uint32_t)(tracked >> 32));
        P.tile_out[pose * (size_t)P.n_tiles + tile] = t;
    }
    }
}

}  // namespace

hipError_t launch_packed_prepare(const PackedPrepareLaunch &p, hipStream_t stream) {
    if (p.n_poses == 0 || p.n_tiles == 0) return hipSuccess;
    const size_t blocks = ((p.n_poses + kPreparePoses - 1) / kPreparePoses) * (size_t)p.n_tiles;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dfire_packed_prepare, dim3((unsigned)blocks), dim3(64), 0, stream, p);
    return hipGetLastError();
}

}  // namespace ld
