// prepare_pdb.hpp -- the cleaned, centred copy of a PDB file a run reads as lightdock_<name>.pdb (lightdock_hip.h,
// "Preparing a run"), host only: the ATOM / HETATM records in file order, hydrogens, OXT and waters dropped unless kept,
// shifted by the mean of the kept atoms in exact integers on thousandths.
#pragma once

#include <cstddef>
#include <cstdint>

namespace ld {

constexpr int kKeepHydrogens = 1, kKeepOxt = 2, kKeepWaters = 4;

struct PreparedPdb {
    size_t atoms = 0;       // records written
    double centre[3] = {0, 0, 0};   // the mean that was subtracted, A
};

// Throws LD_ERR_IO for a file that cannot be read or written or a record shorter than 54 columns, LD_ERR_INVALID for a
// file in which no atom is kept or a shifted coordinate that "%8.3f" cannot hold; the output file is written only after
// every record has passed.
PreparedPdb prepare_pdb(const char *in_path, const char *out_path, int keep_flags);

}  // namespace ld
