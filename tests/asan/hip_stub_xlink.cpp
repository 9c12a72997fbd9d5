// hip_stub_xlink.cpp -- TEST INFRASTRUCTURE for the sanitizer build of the host side (`make asan`, `make asan-xlinks`): the
// launches of kernels/xlink.hpp, beside tests/asan/hip_stub.cpp which stands in for the HIP runtime and every other kernel.
// Device memory is host memory there, so ASan checks every extent below against what xlink.cpp allocated.  The launches do
// their kernels' work in plain C++ from the rule both sides share (xlink_box, xlink_row_span, xlink_isqrt, xlink_square: host
// code too): posing and rounding by the kernel's own kernels/complex_rule.hpp, the blocked nodes of a box row by row, then
// Dijkstra's algorithm with a heap from the source's doors -- no levels, no sub-boxes, no bitmap, so a disagreement with the
// kernel's structure would show.
#include <algorithm>
#include <climits>
#include <cmath>
#include <functional>
#include <queue>
#include <utility>
#include <vector>

#include "kernels/complex_rule.hpp"
#include "kernels/xlink.hpp"
#include "stub_access.hpp"

namespace ld {

hipError_t launch_xlink_straight(const ComplexDevice &m, const double *poses, size_t stride, size_t n, const uint32_t *links, int n_links,
                                 unsigned long long *straight2, int *overflow, hipStream_t) {
    if (n < 1 || n_links < 1 || n_links > kXlinkMaxLinks) return hipErrorInvalidValue;
    peek_complex(m, poses, stride, n);
    peek(links, 2 * (size_t)n_links);
    touch(straight2, n * (size_t)n_links);
    peek(overflow, 1);   // set, never cleared, by the kernel
    for (size_t i = 0; i < n; i++)
        for (int l = 0; l < n_links; l++) {
            if (links[2 * l] >= (uint32_t)(m.n_rec + m.n_lig) || links[2 * l + 1] >= (uint32_t)(m.n_rec + m.n_lig)) return hipErrorInvalidValue;
            int a[3], b[3];
            const bool ok_a = posed_thousandths(m, poses + i * stride, links[2 * l], kComplexCoordBound, a);
            const bool ok_b = posed_thousandths(m, poses + i * stride, links[2 * l + 1], kComplexCoordBound, b);
            if (!ok_a || !ok_b) {
                *overflow |= 1;
                continue;
            }
            straight2[i * (size_t)n_links + l] = xlink_square(a, b);
        }
    return hipSuccess;
}

namespace {

// The distance of every node of `box` from the anchor at c through its doors, up to M; -1 where there is none.
std::vector<int> dijkstra(const XlinkBox &box, const std::vector<char> &blocked, const int c[3], const XlinkDevice &d) {
    const int nx = box.n[0], ny = box.n[1], nz = box.n[2];
    auto at = [&](int i, int j, int k) { return ((size_t)k * ny + j) * nx + i; };
    std::vector<int> dist(blocked.size(), -1);
    typedef std::pair<int, size_t> Item;
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
    for (int k = 0; k < nz; k++)
        for (int j = 0; j < ny; j++)
            for (int i = 0; i < nx; i++) {
                const long long dx = (long long)(box.lo[0] + i) * d.h - c[0], dy = (long long)(box.lo[1] + j) * d.h - c[1],
                                dz = (long long)(box.lo[2] + k) * d.h - c[2];
                const long long d2 = dx * dx + dy * dy + dz * dz;
                if (d2 <= (long long)d.reach * d.reach && !blocked[at(i, j, k)]) heap.push(Item((int)xlink_isqrt(d2), at(i, j, k)));
            }
    const int w[4] = {0, d.h, d.w2, d.w3};
    while (!heap.empty()) {
        const Item top = heap.top();
        heap.pop();
        if (dist[top.second] >= 0 || top.first > d.M) continue;
        dist[top.second] = top.first;
        const int i = (int)(top.second % nx), j = (int)(top.second / nx % ny), k = (int)(top.second / nx / ny);
        for (int dz = -1; dz <= 1; dz++)
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    const int ii = i + dx, jj = j + dy, kk = k + dz;
                    if (ii < 0 || ii >= nx || jj < 0 || jj >= ny || kk < 0 || kk >= nz || (!dx && !dy && !dz)) continue;
                    if (blocked[at(ii, jj, kk)] || dist[at(ii, jj, kk)] >= 0) continue;
                    heap.push(Item(top.first + w[(dx != 0) + (dy != 0) + (dz != 0)], at(ii, jj, kk)));
                }
    }
    return dist;
}

}  // namespace

hipError_t launch_xlink_paths(const ComplexDevice &m, const XlinkDevice &d, const double *poses, size_t stride, size_t n, size_t slots, void *ws,
                              uint32_t *path, int *overflow, hipStream_t) {
    if (n < 1 || d.n_sources < 1 || slots < 1 || slots > (size_t)kXlinkSlots || slots > n * (size_t)d.n_sources) return hipErrorInvalidValue;
    if (d.h < kXlinkMinCell || d.h > kXlinkMaxCell || d.probe < 0 || d.probe > kSasaMaxProbe || d.reach < 1 || d.reach > kXlinkMaxReach) return hipErrorInvalidValue;
    if (d.M < d.h || d.M > kXlinkMaxLength || d.M / d.h > kXlinkMaxSteps) return hipErrorInvalidValue;
    if ((long long)d.w2 * d.w2 > 2ll * d.h * d.h || (long long)(d.w2 + 1) * (d.w2 + 1) <= 2ll * d.h * d.h) return hipErrorInvalidValue;
    if ((long long)d.w3 * d.w3 > 3ll * d.h * d.h || (long long)(d.w3 + 1) * (d.w3 + 1) <= 3ll * d.h * d.h) return hipErrorInvalidValue;
    if (d.n_part < 1 || d.n_links < 1 || d.n_links > kXlinkMaxLinks || d.n_sources > d.n_links) return hipErrorInvalidValue;
    if ((long long)d.n_part * d.rmax * d.rmax > (long long)INT_MAX) return hipErrorInvalidValue;
    peek_complex(m, poses, stride, n);
    peek(d.part_atom, (size_t)d.n_part);
    peek(d.part_radius, (size_t)d.n_part);
    peek(d.source, (size_t)d.n_sources);
    peek(d.first, (size_t)d.n_sources + 1);
    peek(d.target, (size_t)d.n_links);
    peek(d.link, (size_t)d.n_links);
    touch(static_cast<char *>(ws), slots * xlink_slot_bytes(d.n_part, d.M, d.h));   // ws + blockIdx * xlink_slot_bytes
    touch(path, n * (size_t)d.n_links);
    peek(overflow, 1);   // set, never cleared, by the kernel
    const uint32_t n_atoms = (uint32_t)(m.n_rec + m.n_lig);
    // every link answered once, by a source that is one of its anchors
    if (d.first[0] != 0 || d.first[d.n_sources] != (uint32_t)d.n_links) return hipErrorInvalidValue;
    std::vector<char> answered((size_t)d.n_links, 0);
    for (int s = 0; s < d.n_sources; s++) {
        if (d.source[s] >= n_atoms || d.first[s] >= d.first[s + 1]) return hipErrorInvalidValue;
        for (uint32_t e = d.first[s]; e < d.first[s + 1]; e++) {
            if (d.target[e] >= n_atoms || d.link[e] >= (uint32_t)d.n_links || answered[d.link[e]]) return hipErrorInvalidValue;
            answered[d.link[e]] = 1;
        }
    }
    for (int a = 0; a < d.n_part; a++) {
        const uint32_t R = d.part_radius[a];
        if (d.part_atom[a] >= n_atoms || R < 1 || R > (uint32_t)kSasaMaxRadius || 2 * ((int)R + d.probe - 1) / d.h + 1 > d.rmax) return hipErrorInvalidValue;
    }
    std::vector<int4> blockers((size_t)d.n_part);
    for (size_t i = 0; i < n; i++) {
        const double *row = poses + i * stride;
        bool bad = false;
        for (int a = 0; a < d.n_part; a++) {
            int v[3];
            if (!posed_thousandths(m, row, d.part_atom[a], kComplexCoordBound, v)) *overflow |= 1, bad = true;
            blockers[a] = make_int4(v[0], v[1], v[2], (int)d.part_radius[a] + d.probe);
        }
        for (int s = 0; s < d.n_sources && !bad; s++) {
            int c[3];
            if (!posed_thousandths(m, row, d.source[s], kComplexCoordBound, c)) {
                *overflow |= 1, bad = true;
                break;
            }
            const XlinkBox box = xlink_box(c, d.M, d.h);
            if ((size_t)box.padded() > xlink_max_nodes(d.M, d.h)) return hipErrorInvalidValue;
            const int nx = box.n[0], ny = box.n[1], nz = box.n[2];
            std::vector<char> blocked((size_t)nx * ny * nz, 0);
            for (const int4 &p : blockers)
                for (int k = 0; k < nz; k++)
                    for (int j = 0; j < ny; j++) {
                        int lo, hi;
                        if (!xlink_row_span(p.x, p.y, p.z, p.w, (long long)(box.lo[1] + j) * d.h, (long long)(box.lo[2] + k) * d.h, d.h, lo, hi)) continue;
                        for (int i = std::max(lo - box.lo[0], 0); i <= std::min(hi - box.lo[0], nx - 1); i++) blocked[((size_t)k * ny + j) * nx + i] = 1;
                    }
            const std::vector<int> dist = dijkstra(box, blocked, c, d);
            for (uint32_t e = d.first[s]; e < d.first[s + 1]; e++) {
                int b[3];
                if (!posed_thousandths(m, row, d.target[e], kComplexCoordBound, b)) {
                    *overflow |= 1, bad = true;
                    break;
                }
                long long best = LLONG_MAX;
                for (int k = 0; k < nz; k++)
                    for (int j = 0; j < ny; j++)
                        for (int ii = 0; ii < nx; ii++) {
                            const int at = (int)(((size_t)k * ny + j) * nx + ii);
                            if (dist[at] < 0) continue;
                            const long long dx = (long long)(box.lo[0] + ii) * d.h - b[0], dy = (long long)(box.lo[1] + j) * d.h - b[1],
                                            dz = (long long)(box.lo[2] + k) * d.h - b[2];
                            const long long d2 = dx * dx + dy * dy + dz * dz;
                            if (d2 <= (long long)d.reach * d.reach) best = std::min(best, dist[at] + xlink_isqrt(d2));
                        }
                path[i * (size_t)d.n_links + d.link[e]] = best <= d.M ? (uint32_t)best : kXlinkNoPath;
            }
        }
    }
    return hipSuccess;
}

}  // namespace ld
