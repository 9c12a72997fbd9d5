// ranked.hpp -- launch interface of K3e, the clustering of one ranked list of poses in several workgroups
// (kernels/ranked.hip; lightdock_hip.h, "Clustering a ranked list"): what the host side (complex.cpp)
// and the kernels share.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels/cluster.hpp"

namespace ld {

constexpr int kRankedBlock = 64;        // candidates a round: a bit each in a 64-bit mask
constexpr int kRankedGranule = 32;      // atoms between two looks at the partial sum (complex_bsas's early exit)
constexpr int kRankedRows = 3 * kRankedGranule;  // coordinate rows of a granule
constexpr int kRankedPickThreads = 1024;
constexpr int kRankedSweepThreads = 256;
constexpr size_t kRankedWorkspaceBytes = size_t(4) << 30;  // every pose's thousandths stay resident

// The words the host reads back after every round.  Positions are SORTED positions (scoring descending, index ascending).
struct RankedStatus {
    double s_max;          // the largest f64 S with within_cutoff(S); -1 when not even S = 0 passes
    int32_t cursor;        // the first position no round has offered as a candidate yet
    int32_t n_clusters;
    int32_t n_candidates;  // of the last pick; 0: the list is exhausted
    int32_t n_leaders;     // of the last pick
    int32_t overflow;      // set by ranked_pose when a thousandth does not fit an int32
    int32_t rounds;
    int32_t leaders[kRankedBlock];  // the last pick's leaders in creation order
};

// ws: n_walk x 3 x n int32, ws[(3 * a + c) * n + position], position fastest; the walked atoms in walk order (the
// ligand's CA / P first).  state: n cluster ids, -1 while unresolved.  reps: n positions of the leaders in creation order.
struct RankedLaunch {
    int n = 0, n_walk = 0;
    int32_t *state = nullptr, *reps = nullptr;
    RankedStatus *status = nullptr;
};

// Every launch ends by itself: no workgroup waits on another one.

// poses: n rows in sorted order; walk: n_walk complex atom indices; ws as above; sets status->overflow.
hipError_t launch_ranked_pose(const ComplexDevice &m, const double *poses, size_t stride, int n, const uint32_t *walk, int n_walk,
                              int32_t *ws, RankedStatus *status, hipStream_t stream);
// Clears the state and the status and finds s_max for `cutoff` over `n_atoms` atoms (the RMSD's divisor, which may
// exceed n_walk: atoms that cannot move are counted and not walked).  In front of launch_ranked_pose.
hipError_t launch_ranked_begin(const RankedLaunch &r, double cutoff, double n_atoms, hipStream_t stream);
// One workgroup: the first kRankedBlock unresolved positions from the cursor against each other; leaders, joins, cursor.
hipError_t launch_ranked_pick(const RankedLaunch &r, const int32_t *ws, hipStream_t stream);
// A lane a position from `from` (a lower bound of the cursor the pick left) on: the unresolved ones behind the cursor
// against the leaders of the last pick.
hipError_t launch_ranked_sweep(const RankedLaunch &r, const int32_t *ws, int from, hipStream_t stream);

}  // namespace ld
