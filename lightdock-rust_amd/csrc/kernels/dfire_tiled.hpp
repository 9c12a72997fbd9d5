// dfire_tiled.hpp -- the tile order the culled DFIRE kernels share (K1, DFIRE): the pose-major kernel
// (dfire_packed.hpp) and the block-major path (dfire_bm.hpp).
//
// Atoms arrive in the spatial tile order of host/spatial_order.hpp: tiles of 64 atoms, subtiles of 8,
// each with a bounding box, so that whole 64x64 and 8x8 blocks of atom pairs whose boxes are further
// apart than the 15 A cutoff can be skipped.  This header holds that order's records and boxes, the
// patch layout of the potential, and the receptor image both culled paths build (dfire_tiled.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "pose_energy.hpp"

namespace ld {

// The culled kernels read the potential in 128-byte patches of 2 ligand types x 2 receptor types
// x 4 distance bins:
//   index = ((l/2)*85 + r/2)*96 + (bin/4)*16 + (l%2)*8 + (r%2)*4 + bin%4        (bin 0..20; 169 types -> 85 pairs)
// The atoms of a subtile are mostly one residue, whose DFIRE types are consecutive numbers, and
// bonded atoms sit in the same or the next distance bin of a given partner, so the hits of one
// 8x8 block fall into fewer distinct cache lines than with any row-major order (simulated on the
// 1k4c poses: 0.63 lines per hit; [lig][bin][rec] rows 0.77, the reference's [rec][lig][bin] 0.95).
// Bin 20 is what the reference reads for r = 15.0 A exactly: potential[r*3380 + l*20 + 20]
// (src/dfire.rs:338).
constexpr uint32_t kTiledTableBins = 21;
constexpr uint32_t kTiledPatchDoubles = 16;                       // one 128-byte line
constexpr uint32_t kTiledRecStride = 6 * kTiledPatchDoubles;      // 24 bin slots per type pair
constexpr uint32_t kTiledLigStride = 85 * kTiledRecStride;        // 169 types -> 85 pairs
constexpr uint32_t kTiledTableDoubles = 85 * kTiledLigStride;
// The three terms are BYTE offsets; their sum is the buffer-load offset of the table entry.
__host__ __device__ inline uint32_t tiled_lig_term(uint32_t type) { return 8u * ((type >> 1) * kTiledLigStride + (type & 1u) * 8u); }
__host__ __device__ inline uint32_t tiled_rec_term(uint32_t type) { return 8u * ((type >> 1) * kTiledRecStride + (type & 1u) * 4u); }
__host__ __device__ inline uint32_t tiled_bin_term(uint32_t bin) { return 8u * (bin + 12u * (bin >> 2)); }

// f32 bounding box rounded outwards; an empty box has lo = +inf, hi = -inf.
struct alignas(16) TiledBox {
    float lox, loy, loz, pad0;
    float hix, hiy, hiz, pad1;
};
static_assert(sizeof(TiledBox) == 32, "TiledBox must be 32 bytes");

// The ligand in tile order, SoA, padded to whole tiles (the kernel re-places padding after posing).
struct TiledLigand {
    int n_real = 0;
    int n_tiles = 0;
    const double *x = nullptr, *y = nullptr, *z = nullptr;
    const uint32_t *tindex = nullptr;
    const int32_t *slot = nullptr;
    int num_anm = 0;
    const double *modes = nullptr;  // [mode][xyz][n_tiles*64]
    int flag_words = 0;
};

// Two receptor atoms as one lane of the pair loop reads them: the atoms (2 q, 2 q + 1) of subtile j
// of a tile (record index 4 j + q).  The operands of v_pk_add_f32 / v_pk_fma_f32 are (x0, x1),
// (y0, y1), (z0, z1) as they lie here.
struct alignas(32) PackedRecPair {
    float x0, x1, y0, y1, z0, z1;
    uint32_t t0, t1;  // tiled_rec_term(type): byte offset of the type's column in a table patch
};
static_assert(sizeof(PackedRecPair) == 32, "PackedRecPair must be 32 bytes");

// The receptor image in the f32 frame of dfire_packed.hpp: pair records, subtile and tile boxes.  Static
// (built once) for a rigid receptor; with receptor ANM one image per pose (src/dfire.rs:304-320).
struct PackedPrepareLaunch {
    int n_real = 0, n_tiles = 0;
    const double *x = nullptr, *y = nullptr, *z = nullptr;  // tile order, padded
    const uint32_t *tindex = nullptr;
    const int32_t *slot = nullptr;
    int num_anm = 0;
    const double *modes = nullptr;  // [mode][xyz][n_tiles*64]
    const double *poses = nullptr;
    size_t stride = 0;
    const uint8_t *active = nullptr;
    size_t n_poses = 0;
    double cx = 0, cy = 0, cz = 0;
    double kappa = 2.0;
    float ubound = 0.f;
    PackedRecPair *pairs_out = nullptr;
    TiledBox *sub_out = nullptr, *tile_out = nullptr;
};

hipError_t launch_packed_prepare(const PackedPrepareLaunch &p, hipStream_t stream);

}  // namespace ld
