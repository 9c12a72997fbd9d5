// emfit.hpp -- the host side of the density fit (lightdock_hip.h, "Density fit"): a quantised map and its
// device copy, the kernel table the host makes with libm, and the scores.  What the header says of ld_density_* holds for
// the functions of the same names; refusals are ld::Error.  The methods of Complex that use them (density_fit,
// simulate_density) are defined in emfit.cpp too.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "device_memory.hpp"
#include "kernels/emfit.hpp"

namespace ld {

// The table of a sigma: K[t], t < length, and the shift.
struct DensityKernel {
    std::vector<uint32_t> table;
    uint32_t shift = 0;
    uint32_t limit() const { return (uint32_t)table.size() << shift; }  // T << s, below 2^32
    uint32_t reach() const;                                             // isqrt(limit - 1)
};
DensityKernel density_kernel(uint32_t sigma);
// floor(sqrt(v)), exactly.
uint32_t isqrt64(unsigned long long v);

class Density {
   public:
    Density(const float *rho, const uint32_t n[3], const int32_t origin[3], const uint32_t step[3], double threshold);
    Density(const Density &) = delete;
    Density &operator=(const Density &) = delete;

    size_t voxels() const { return E_.size(); }
    uint64_t s_e() const { return s_e_; }
    uint64_t s_ee() const { return s_ee_; }
    double scale() const { return scale_; }
    const std::vector<uint16_t> &E() const { return E_; }
    int min_step() const;
    // The map as the kernels read it; the voxels are uploaded by the first call.
    EmfitMap device();
    void scores(size_t n, const ld_density_sums *sums, double *cc, double *ccm, double *inside) const;

   private:
    EmfitMap map_;
    std::vector<uint16_t> E_;
    uint64_t s_e_ = 0, s_ee_ = 0;
    double scale_ = 0.0;
    DeviceBuffer d_E_;
};

}  // namespace ld

struct ld_density {
    ld::Density impl;
    ld_density(const float *rho, const uint32_t n[3], const int32_t origin[3], const uint32_t step[3], double threshold)
        : impl(rho, n, origin, step, threshold) {}
};
