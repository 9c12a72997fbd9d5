// ranked_host.hpp -- TEST INFRASTRUCTURE of the sanitizer build around the ranked clustering (`make asan-ranked`): the posing
// of one atom, the thousandths "%8.3f" prints and the clustering's RMSD test in plain C++, as kernels/complex_rule.hpp and kernels/complex_pose.hpp
// state them for the device.  tests/asan/hip_stub_ranked.cpp poses with it in place of the kernel, and the driver
// (tests/asan/ranked_check.cpp) poses with it for its sequential loop, so what the two compare is the clustering.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "kernels/cluster.hpp"

namespace ranked_host {

inline double thousandths(double x) {
    const double p = x * 1000.0;
    const double e = std::fma(x, 1000.0, -p);
    const double f = std::floor(p);
    if (p - f == 0.5) {
        if (e > 0.0) return f + 1.0;
        if (e < 0.0) return f;
    }
    return std::rint(p);
}

inline bool within_cutoff(double S, double n, double cutoff) { return std::rint(std::sqrt(S * 1e-6 / n) * 1e4) / 1e4 <= cutoff; }

// Complex atom `atom` (receptor atoms first) at the pose in `row`: receptor R + sum ext * mode; ligand
// rotate(q, L + sum ext * mode) + t.
inline void pose_atom(const ld::ComplexDevice &m, const double *row, uint32_t atom, double out[3]) {
    if ((int)atom < m.n_rec) {
        for (int c = 0; c < 3; c++) out[c] = m.rec_xyz[3 * (size_t)atom + c];
        for (int k = 0; k < m.anm_rec; k++)
            for (int c = 0; c < 3; c++) out[c] += m.rec_modes[((size_t)k * m.n_rec + atom) * 3 + c] * row[7 + k];
        return;
    }
    const uint32_t a = atom - (uint32_t)m.n_rec;
    double v[3];
    for (int c = 0; c < 3; c++) v[c] = m.lig_xyz[3 * (size_t)a + c];
    for (int k = 0; k < m.anm_lig; k++)
        for (int c = 0; c < 3; c++) v[c] += m.lig_modes[((size_t)k * m.n_lig + a) * 3 + c] * row[7 + m.anm_rec + k];
    const double qw = row[3], qx = row[4], qy = row[5], qz = row[6];
    const double aw = qw * 0.0 - qx * v[0] - qy * v[1] - qz * v[2];
    const double ax = qw * v[0] + qx * 0.0 + qy * v[2] - qz * v[1];
    const double ay = qw * v[1] - qx * v[2] + qy * 0.0 + qz * v[0];
    const double az = qw * v[2] + qx * v[1] - qy * v[0] + qz * 0.0;
    const double n2 = qw * qw + qx * qx + qy * qy + qz * qz;
    const double bw = qw / n2, bx = -qx / n2, by = -qy / n2, bz = -qz / n2;
    out[0] = aw * bx + ax * bw + ay * bz - az * by + row[0];
    out[1] = aw * by - ax * bz + ay * bw + az * bx + row[1];
    out[2] = aw * bz + ax * by - ay * bx + az * bw + row[2];
}

}  // namespace ranked_host
