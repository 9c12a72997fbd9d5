#include "prepare_pdb.hpp"

#include <cmath>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "error.hpp"
#include "kernels/sasa.hpp"
#include "pdb_file.hpp"

namespace ld {

namespace {

std::string trimmed(const std::string &s) {
    const size_t b = s.find_first_not_of(' ');
    return b == std::string::npos ? std::string() : s.substr(b, s.find_last_not_of(' ') - b + 1);
}

}  // namespace

PreparedPdb prepare_pdb(const char *in_path, const char *out_path, int keep_flags) {
    if (!in_path || !out_path) throw Error(LD_ERR_INVALID, "PDB path missing");
    const PdbFile pdb = read_pdb_file_order(in_path);   // refuses a short record
    std::vector<size_t> kept;
    std::vector<long long> t;   // thousandths of the kept atoms, x y z
    long long sum[3] = {0, 0, 0};
    for (size_t a = 0; a < pdb.lines.size(); a++) {
        const std::string &line = pdb.lines[a];
        const std::string res = trimmed(line.substr(17, 3)), name = trimmed(line.substr(12, 4));
        const bool bead = res == "MMB";
        const bool hydrogen = !bead && sasa_radius(line.data(), line.size()) == 0;   // the surface rule's element test
        if (hydrogen && !(keep_flags & kKeepHydrogens)) continue;
        if (name == "OXT" && !(keep_flags & kKeepOxt)) continue;
        if ((res == "HOH" || res == "WAT") && !(keep_flags & kKeepWaters)) continue;
        for (int c = 0; c < 3; c++) {
            const double v = pdb.xyz[3 * a + c];
            if (!(std::fabs(v) < 1.0e6)) throw Error(LD_ERR_INVALID, std::string(in_path) + ": a coordinate beyond +-1.0e6 A");
            const long long q = std::llrint(v * 1000.0);
            t.push_back(q);
            sum[c] += q;
        }
        kept.push_back(a);
    }
    if (kept.empty()) throw Error(LD_ERR_INVALID, std::string(in_path) + ": no atom is kept");
    const long long n = (long long)kept.size();
    std::string text;
    for (size_t k = 0; k < kept.size(); k++) {
        const std::string &line = pdb.lines[kept[k]];
        char field[3][32];
        for (int c = 0; c < 3; c++) {
            // round((t n - sum) / n) to the nearest, halves up: floor((2 (t n - sum) + n) / (2 n)), exact
            const long long num = 2 * (t[3 * k + c] * n - sum[c]) + n, den = 2 * n;
            const long long shifted = num / den - ((num % den != 0 && num < 0) ? 1 : 0);
            if (std::snprintf(field[c], sizeof field[c], "%8.3f", (double)shifted / 1000.0) != 8)
                throw Error(LD_ERR_INVALID, std::string(in_path) + ": a centred coordinate does not fit \"%8.3f\"");
        }
        text += line.substr(0, 30) + field[0] + field[1] + field[2] + line.substr(54) + "\n";
    }
    std::ofstream out(out_path, std::ios::binary);
    if (!out) throw Error(LD_ERR_IO, std::string("cannot write ") + out_path);
    out.write(text.data(), (std::streamsize)text.size());
    out.close();
    if (!out) throw Error(LD_ERR_IO, std::string("cannot write ") + out_path);
    PreparedPdb result;
    result.atoms = kept.size();
    for (int c = 0; c < 3; c++) result.centre[c] = (double)sum[c] / (double)n / 1000.0;
    return result;
}

}  // namespace ld
