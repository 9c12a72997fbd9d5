#include "pdb_file.hpp"

#include <cstdlib>
#include <fstream>

#include "error.hpp"

namespace ld {

namespace {

std::string trimmed(const std::string &s) {
    const size_t b = s.find_first_not_of(' ');
    return b == std::string::npos ? std::string() : s.substr(b, s.find_last_not_of(' ') - b + 1);
}

// Fills res_start, res_of_atom and res_id from `lines` (every line has 54 columns at least).
void cut_residues(PdbFile &f) {
    for (size_t a = 0; a < f.lines.size(); a++) {
        const std::string &line = f.lines[a];
        // resname; chain, serial, icode
        if (a == 0 || line.compare(17, 3, f.lines[a - 1], 17, 3) != 0 || line.compare(21, 6, f.lines[a - 1], 21, 6) != 0) {
            f.res_start.push_back((uint32_t)a);
            f.res_id.push_back(trimmed(line.substr(21, 1)) + "." + trimmed(line.substr(17, 3)) + "." +
                               std::to_string(std::strtol(line.substr(22, 4).c_str(), nullptr, 10)) + trimmed(line.substr(26, 1)));
        }
        f.res_of_atom.push_back((uint32_t)f.res_id.size() - 1);
    }
    f.res_start.push_back((uint32_t)f.lines.size());
}

}  // namespace

PdbFile read_pdb_file_order(const char *path) {
    if (!path) throw Error(LD_ERR_INVALID, "PDB path missing");
    std::ifstream in(path);
    if (!in) throw Error(LD_ERR_IO, std::string("cannot open PDB file ") + path);
    PdbFile f;
    std::string line;
    while (std::getline(in, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.compare(0, 6, "ATOM  ") != 0 && line.compare(0, 6, "HETATM") != 0) continue;
        if (line.size() < 54) throw Error(LD_ERR_IO, std::string(path) + ": ATOM/HETATM record shorter than 54 columns");
        for (int k = 0; k < 3; k++) {
            const std::string field = line.substr(30 + 8 * k, 8);
            char *end = nullptr;
            const double v = std::strtod(field.c_str(), &end);
            if (end == field.c_str()) throw Error(LD_ERR_IO, std::string(path) + ": unreadable coordinate '" + field + "'");
            f.xyz.push_back(v);
        }
        std::string name = line.substr(12, 4);
        name.erase(name.find_last_not_of(' ') + 1);
        name.erase(0, name.find_first_not_of(' '));
        if (name == "CA" || name == "P") f.backbone.push_back((uint32_t)f.lines.size());
        f.lines.push_back(line);
    }
    if (f.lines.empty()) throw Error(LD_ERR_INVALID, std::string(path) + ": no ATOM/HETATM records");
    cut_residues(f);
    return f;
}

}  // namespace ld
