// decompose.hpp -- the host object behind ld_scorer_decompose (include/lightdock_hip.h "Energy decomposition"): both
// molecules in the reference's atom order on the device, the grow-only workspace of a pass, the passes of a call.
// Reached through an `ld_scorer*`, which keeps a deep copy of the description it was made from and builds this on first use.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "device_memory.hpp"
#include "kernels/decompose.hpp"
#include "lightdock_hip.h"

namespace ld {

// A scorer description that owns its arrays.
class DescCopy {
   public:
    explicit DescCopy(const ld_scorer_desc &d);
    DescCopy(const DescCopy &) = delete;
    DescCopy &operator=(const DescCopy &) = delete;
    const ld_scorer_desc &view() const { return desc_; }

   private:
    struct Molecule {
        std::vector<double> coordinates, ele_charges, vdw_charges, vdw_radii, nmodes;
        std::vector<uint32_t> dfire_types, membrane, restraint_offsets, restraint_atoms;
    };
    void copy(const ld_molecule &from, Molecule &store, ld_molecule &to);
    Molecule rec_, lig_;
    std::vector<double> potential_;
    ld_scorer_desc desc_;
};

class Decomposer {
   public:
    // desc: checked by the scorer it comes from (method DFIRE, DNA or PYDOCK)
    explicit Decomposer(const ld_scorer_desc &desc);
    Decomposer(const Decomposer &) = delete;
    Decomposer &operator=(const Decomposer &) = delete;
    ~Decomposer();

    static size_t slice_of(const ld_scorer_desc &desc);   // poses per pass: host arithmetic only
    size_t slice() const { return slice_; }
    size_t pose_len() const { return 7 + (size_t)model_.rec.num_anm + (size_t)model_.lig.num_anm; }
    double last_kernel_ms() const { return last_ms_; }

    // ld_scorer_decompose: every refusal is thrown before anything is launched or written.  Synchronous on `stream`.
    void run(size_t n, const double *poses, size_t stride, ld_energy_terms *terms_out, const ld_group_energies *receptor,
             const ld_group_energies *ligand, hipStream_t stream);

   private:
    struct SideGroups {   // one side of one call
        bool wanted = false;
        size_t n_groups = 0;
        std::vector<uint32_t> offsets, atoms;
        DeviceBuffer d_offsets, d_atoms, d_sums, d_pairs, d_iface;
    };
    DecomposeMolecule upload(const ld_molecule &m, int method, bool is_receptor, bool use_anm);
    void check_groups(const ld_group_energies *g, int side, size_t n, SideGroups &out) const;

    DeviceArena arena_;
    DecomposeLaunch model_;   // molecule and table pointers, filled once; pass fields per run()
    DecomposeTail tail_;
    size_t slice_ = 1;
    DeviceBuffer ws_, ws_poses_, ws_terms_;
    SideGroups groups_[2];
    hipEvent_t start_ = nullptr, stop_ = nullptr;
    double last_ms_ = 0.0;
};

}  // namespace ld
