// pdb_file.hpp -- a PDB file as the analysis half of a run reads it (complex.hpp): the ATOM / HETATM records kept as
// text and in FILE order, because LightDock's tools pose and rewrite the records of the file as they stand.
//
// Deliberately not read_pdb of structure.hpp: that one gives the scoring functions pdbtbx's chain -> residue -> atom walk
// and skips short records silently, this one keeps the file's order and refuses them.  Its residue ids follow the same
// "<chain>.<resname>.<serial><icode>" rule as AtomRecord::residue_id() but trim blanks only, where structure.cpp's fields
// also trim tabs: the strings differ for a tab in those columns, so neither the rule nor the trimming helper is shared.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace ld {

struct PdbFile {
    std::vector<std::string> lines;  // ATOM / HETATM records as read (other records are dropped)
    std::vector<double> xyz;
    std::vector<uint32_t> backbone;  // atoms named CA or P
    // residues: maximal runs of consecutive records with the same columns 18-20, 22, 23-26 and 27
    std::vector<uint32_t> res_start;     // first atom of each residue, then the atom count
    std::vector<uint32_t> res_of_atom;
    std::vector<std::string> res_id;     // "<chain>.<resname>.<serial><icode>", AtomRecord::residue_id() (src/dfire.rs:139-142)
};

// Throws ld::Error: LD_ERR_INVALID for a null path or a file without ATOM / HETATM records, LD_ERR_IO for a file that
// cannot be opened, a record shorter than 54 columns or an unreadable coordinate.  A trailing '\r' is stripped.
PdbFile read_pdb_file_order(const char *path);

}  // namespace ld
