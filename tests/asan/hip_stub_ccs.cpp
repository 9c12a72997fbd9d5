// hip_stub_ccs.cpp -- TEST INFRASTRUCTURE for the sanitizer build of the host side (`make asan`, `make asan-ccs`): the
// launches of kernels/ccs.hpp, beside tests/asan/hip_stub.cpp which stands in for the HIP runtime and every other kernel.
// Device memory is host memory there, so ASan checks every extent below against what ccs.cpp allocated.  The launches do
// their kernels' work in plain C++ from the rule both sides share (ccs_project, ccs_row_span, ccs_box, kCcsFrames: host code
// too): posing and rounding by the kernel's own kernels/complex_rule.hpp, then every view row by row -- the atoms'
// column intervals of a row merged and counted, the rigid receptor's bits of that row added where no interval holds them.
// No pieces and no LDS bitmap, so a disagreement with the kernel's structure would show.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "kernels/complex_rule.hpp"
#include "kernels/ccs.hpp"
#include "stub_access.hpp"

namespace ld {

typedef std::map<int, std::vector<std::pair<int, int>>> Rows;   // row j -> the column intervals of the atoms

// The intervals of view v of `atoms` (x, y, z, E), added to `rows`; the extremes of the discs folded into ext (lo a, hi a, lo b, hi b).
static void add_atoms(const int4 *atoms, int n, int v, int h, Rows &rows, int ext[4]) {
    for (int k = 0; k < n; k++) {
        const int4 &p = atoms[k];
        const int a = ccs_project(kCcsFrames[v], p.x, p.y, p.z), b = ccs_project(kCcsFrames[v] + 3, p.x, p.y, p.z);
        ext[0] = std::min(ext[0], a - p.w), ext[1] = std::max(ext[1], a + p.w);
        ext[2] = std::min(ext[2], b - p.w), ext[3] = std::max(ext[3], b + p.w);
        for (int j = ccs_ceil_div(b - p.w, h); j <= ccs_floor_div(b + p.w, h); j++) {
            int lo, hi;
            if (ccs_row_span(a, b, p.w, j, h, lo, hi)) rows[j].push_back(std::make_pair(lo, hi));
        }
    }
}

hipError_t launch_ccs_receptor(const int4 *atoms, int n_atoms, int h, int rmax, const CcsRecView *views, uint32_t *rec_bits, hipStream_t) {
    if (n_atoms < 1 || h < kCcsMinCell || h > kCcsMaxCell || rmax < 1 || (long long)n_atoms * rmax > (long long)INT_MAX) return hipErrorInvalidValue;
    peek(atoms, (size_t)n_atoms);
    peek(views, (size_t)kCcsViews);
    for (int v = 0; v < kCcsViews; v++) {
        const CcsRecView &w = views[v];
        if (w.pitch < 1 || w.rows < 1) return hipErrorInvalidValue;
        uint32_t *bits = rec_bits + w.offset;
        peek(bits, (size_t)w.pitch * (size_t)w.rows);   // ZEROED by the caller: read, not cleared
        Rows rows;
        int ext[4] = {INT_MAX, INT_MIN, INT_MAX, INT_MIN};
        add_atoms(atoms, n_atoms, v, h, rows, ext);
        if (ext[0] != w.lo_a || ext[1] != w.hi_a || ext[2] != w.lo_b || ext[3] != w.hi_b) return hipErrorInvalidValue;
        for (const auto &row : rows) {
            if (row.first < w.j0 || row.first >= w.j0 + w.rows || (int)row.second.size() > n_atoms) return hipErrorInvalidValue;
            for (const auto &span : row.second)
                for (int i = span.first; i <= span.second; i++) {
                    const int k = (i >> 5) - w.wc0;
                    if (k < 0 || k >= w.pitch) return hipErrorInvalidValue;
                    bits[(size_t)(row.first - w.j0) * (size_t)w.pitch + (size_t)k] |= 1u << (i & 31);
                }
        }
    }
    return hipSuccess;
}

hipError_t launch_complex_ccs(const ComplexDevice &m, const CcsDevice &d, const double *poses, size_t stride, size_t n, size_t slots, void *ws,
                              uint32_t *counts, unsigned long long *sums, int *overflow, hipStream_t) {
    if (slots < 1 || slots > (size_t)kCcsSlots || slots > n) return hipErrorInvalidValue;
    if (d.h < kCcsMinCell || d.h > kCcsMaxCell || d.probe < 0 || d.probe > kSasaMaxProbe) return hipErrorInvalidValue;
    if (d.first < 0 || d.count < 1 || d.rmax < 2 * kSasaMaxRadius / kCcsMaxCell || (long long)d.count * d.rmax > (long long)INT_MAX) return hipErrorInvalidValue;
    if ((d.rec_views == nullptr) != (d.rec_bits == nullptr)) return hipErrorInvalidValue;
    const bool rigid = d.rec_bits != nullptr;
    if (rigid && m.anm_rec != 0) return hipErrorInvalidValue;
    peek_complex(m, poses, stride, n);
    peek(d.part_atom + d.first, (size_t)d.count);
    peek(d.part_radius + d.first, (size_t)d.count);
    touch(static_cast<char *>(ws), slots * ccs_slot_bytes(d.count));   // ws + blockIdx * ccs_slot_bytes
    touch(counts, n * (size_t)kCcsViews);
    touch(sums, n);
    peek(overflow, 1);   // set, never cleared, by the kernel
    if (rigid) peek(d.rec_views, (size_t)kCcsViews);
    for (int a = 0; a < d.count; a++) {
        const uint32_t atom = d.part_atom[d.first + a], R = d.part_radius[d.first + a];
        if (atom >= (uint32_t)(m.n_rec + m.n_lig) || (a && atom <= d.part_atom[d.first + a - 1])) return hipErrorInvalidValue;
        if (rigid && atom < (uint32_t)m.n_rec) return hipErrorInvalidValue;   // the receptor is in the bitmaps
        if (R < 1 || R > (uint32_t)kSasaMaxRadius || 2 * ((int)R + d.probe) / d.h + 1 > d.rmax) return hipErrorInvalidValue;
    }
    std::vector<int4> atoms((size_t)d.count);
    for (size_t i = 0; i < n; i++) {
        const double *row = poses + i * stride;
        bool bad = false;
        for (int a = 0; a < d.count; a++) {
            int v[3];
            if (!posed_thousandths(m, row, d.part_atom[d.first + a], kComplexCoordBound, v)) *overflow |= 1, bad = true;
            atoms[a] = make_int4(v[0], v[1], v[2], (int)d.part_radius[d.first + a] + d.probe);
        }
        unsigned long long total = 0;
        for (int v = 0; v < kCcsViews && !bad; v++) {
            Rows rows;
            int ext[4] = {INT_MAX, INT_MIN, INT_MAX, INT_MIN};
            add_atoms(atoms.data(), d.count, v, d.h, rows, ext);
            const CcsRecView *w = rigid ? &d.rec_views[v] : nullptr;
            if (w) ext[0] = std::min(ext[0], w->lo_a), ext[1] = std::max(ext[1], w->hi_a), ext[2] = std::min(ext[2], w->lo_b), ext[3] = std::max(ext[3], w->hi_b);
            const CcsBox box = ccs_box(ext[0], ext[1], ext[2], ext[3], d.h);
            if (box.columns() * box.rows() > kCcsMaxBox) {
                *overflow |= 2, bad = true;
                break;
            }
            if (w)
                for (int r = 0; r < w->rows; r++) rows[w->j0 + r];   // a row of the receptor's alone is counted too
            unsigned long long count = 0;
            for (auto &row : rows) {
                std::vector<std::pair<int, int>> &s = row.second;
                std::sort(s.begin(), s.end());
                std::vector<std::pair<int, int>> merged;
                for (const auto &span : s) {
                    if (!merged.empty() && span.first <= merged.back().second + 1) merged.back().second = std::max(merged.back().second, span.second);
                    else merged.push_back(span);
                }
                for (const auto &span : merged) count += (unsigned long long)(span.second - span.first + 1);
                if (!w || row.first < w->j0 || row.first >= w->j0 + w->rows) continue;
                const uint32_t *bits = d.rec_bits + w->offset + (size_t)(row.first - w->j0) * (size_t)w->pitch;
                peek(bits, (size_t)w->pitch);
                for (int k = 0; k < w->pitch; k++)
                    for (int bit = 0; bit < 32; bit++) {
                        if (!(bits[k] >> bit & 1)) continue;
                        const int col = (w->wc0 + k) * 32 + bit;
                        bool held = false;
                        for (const auto &span : merged) held = held || (col >= span.first && col <= span.second);
                        if (!held) count++;
                    }
            }
            counts[i * (size_t)kCcsViews + v] = (uint32_t)count;
            total += count;
        }
        if (!bad) sums[i] = total;
    }
    return hipSuccess;
}

}  // namespace ld
