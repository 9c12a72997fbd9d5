// fcc.hpp -- the host side of clustering by common contacts (include/lightdock_hip.h, "Clustering by common contacts";
// DESIGN §5 K3g): the launch sequence of kernels/fcc.hpp on sets that are on the device already, with its grow-only
// workspace, and the entries that take their sets from the caller.  ld::Complex owns one FccCluster for
// ld_complex_cluster_fcc, whose sets never leave the device; ld_fcc_common / ld_fcc_cluster build one for the call.
#pragma once

#include <cstdint>
#include <vector>

#include "device_memory.hpp"
#include "kernels/fcc.hpp"

namespace ld {

// T = llrint(threshold * 1000), 1 .. 1000; anything else, a NaN included, is refused.
uint32_t fcc_threshold(double threshold);

class FccCluster {
   public:
    // n sets in CSR form on the device; every key lies in [key_lo, key_lo + key_span).
    struct Sets {
        size_t n = 0, total = 0;
        const uint32_t *d_offsets = nullptr, *d_keys = nullptr;
        uint32_t key_lo = 0;
        uint64_t key_span = 1;
    };
    struct Result {
        std::vector<int32_t> cluster_of, centres;  // n each, in input order; centres: -1 after the last
        uint32_t n_clusters = 0, rounds = 0;
        std::vector<uint64_t> consensus;  // n, or empty
    };
    // Everything is queued on `stream` and synchronised before the call returns.  n >= 1; scoring is finite.
    void cluster(const Sets &s, const double *scoring, uint32_t T, uint32_t min_size, bool consensus, hipStream_t stream, Result &out);
    void common(const Sets &s, uint32_t *common_out, hipStream_t stream);

   private:
    size_t build_rows(const Sets &s, const uint32_t *d_row_of, hipStream_t stream);  // -> W, the words of a bit row

    DeviceBuffer status_, bitmap_, rank_, rows_, cols_, freq_, sizes_, work_, nbr_, out_;
};

// ld_fcc_common / ld_fcc_cluster: the caller's sets, checked, uploaded and run on the null stream.
void fcc_common_host(size_t n, const uint32_t *offsets, const uint32_t *keys, uint32_t *common);
void fcc_cluster_host(size_t n, const uint32_t *offsets, const uint32_t *keys, const double *scoring, double threshold,
                      uint32_t min_size, int32_t *cluster_of, int32_t *centres, uint32_t *n_clusters, uint64_t *consensus);
double fcc_last_kernel_ms();

}  // namespace ld
