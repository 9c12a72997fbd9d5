// sasa.hpp -- launch interface of K3f, the solvent-accessible surface of every pose (kernels/sasa.hip; DESIGN §5 K3f;
// lightdock_hip.h, "Solvent-accessible surface"): what the host side (complex.cpp) and the kernel share, and the integer
// rule itself (radii, directions, a point's offset, the burial test), which is host code too so that a CPU build restates it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels/cluster.hpp"
#include "lightdock_hip.h"

namespace ld {

constexpr int kSasaPoints = LD_SASA_POINTS;  // two points a lane
constexpr int kSasaThreads = 512;
constexpr int kSasaSlots = kContactSlots;
constexpr int kSasaCells = 4096;             // cells of ONE molecule's grid; both grids' offsets are 32 KiB of LDS
constexpr int kSasaListCap = 128;            // neighbours a wave keeps in LDS before it tests its points against them
constexpr int kSasaMaxProbe = 2000;          // thousandths
constexpr int kSasaMaxRadius = 1980;         // the largest radius of the table
// A point of atom a lies within E_a + 1 of c_a (a rounded direction is at most 0.87 / 2^20 longer than a unit vector, a
// rounded offset at most 0.87 off), so an atom b can bury a point of a only if |c_a - c_b| < E_a + E_b + kSasaSlack.
constexpr int kSasaSlack = 1;

// --- the rule, on integers (thousandths) ------------------------------------------------------------------------------

// 128 x 3: rint(2^20 * unit vector) of the golden spiral (tools/gen_sasa_directions.py)
inline constexpr int32_t kSasaDirections[kSasaPoints][3] = {
#include "kernels/sasa_directions.inc"
};

// One component of point k's offset from the centre of an atom of expanded radius E: (E U + 2^19) >> 20, arithmetic.
__host__ __device__ inline int sasa_offset(int E, int u) { return (int)(((long long)E * u + (1ll << 19)) >> 20); }

// Point c_a + off is buried by the atom at c_a + rel of squared expanded radius E2: |off - rel|^2 < E2, strictly.  The
// caller knows |rel| <= 2 * (kSasaMaxRadius + kSasaMaxProbe) + kSasaSlack and |off| <= E_a + 1: every term fits 32 bits.
__host__ __device__ inline bool sasa_buried(int ox, int oy, int oz, int rx, int ry, int rz, int E2) {
    const int dx = ox - rx, dy = oy - ry, dz = oz - rz;
    return dx * dx + dy * dy + dz * dz < E2;
}

// The radius in thousandths of an ATOM / HETATM record, 0 for a record that takes no part: hydrogen, deuterium, or a
// residue named MMB.  The element: columns 77-78, trimmed and upper-cased; a record too short for them or a blank field:
// the first alphabetic character of columns 13-16.  `line` has 54 columns at least.
uint32_t sasa_radius(const char *line, size_t len);

struct SasaDevice {
    int n_atoms = 0;             // all atoms of the complex: the row length of the per-atom counts
    int n_part = 0, n_part_rec = 0;  // atoms that take part, the receptor's first
    int e_max = 0;               // the largest expanded radius of the call, R_max + p
    int probe = 0;               // p, thousandths
    const uint32_t *part_atom = nullptr;    // n_part complex atom indices, ascending
    const uint32_t *part_radius = nullptr;  // n_part radii R, thousandths
};

// A workspace slot: the posed atoms, the atoms ordered by cell (int4 x, y, z, E each) and the order's atom numbers.
inline size_t sasa_slot_bytes(int n_part) { return ((size_t)n_part * (2 * sizeof(int4) + sizeof(int)) + 15) / 16 * 16; }

// `slots` workgroups, 1 .. kSasaSlots.  Reads `m` as ComplexDevice says and pose rows of 7 + m.anm_rec + m.anm_lig doubles,
// `stride` doubles apart.  ws: slots x sasa_slot_bytes(d.n_part); sums: n x 4; free_counts, bound_counts: n x d.n_atoms
// bytes each, ZEROED by the caller (only atoms that take part are written), or both null; overflow: one int, set when a
// posed coordinate is beyond +-1.0e6 A.
hipError_t launch_complex_sasa(const ComplexDevice &m, const SasaDevice &d, const double *poses, size_t stride, size_t n,
                               size_t slots, void *ws, unsigned long long *sums, uint8_t *free_counts, uint8_t *bound_counts,
                               int *overflow, hipStream_t stream);

}  // namespace ld
