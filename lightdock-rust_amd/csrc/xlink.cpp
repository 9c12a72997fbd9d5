// xlink.cpp -- the host side of the cross-links (lightdock_hip.h, "Cross-links"): Complex::crosslinks -- the
// argument checks, the grouping of the links by source anchor, the chunking (chunk_of), the workspace (every block laid out
// through device_memory.hpp's Carver) and the launches of kernels/xlink.hpp.
#include <algorithm>
#include <climits>
#include <cmath>
#include <map>
#include <vector>

#include "complex.hpp"
#include "kernels/xlink.hpp"

namespace ld {

namespace {

const char *const kXlinkOverflow = "a posed blocker or anchor is beyond +-1.0e6 A";

// llrint(1000 x) when it lies in lo .. hi, `message` otherwise (a NaN and an infinity too).
int thousandths_in(double x, int lo, int hi, const char *message) {
    if (!(x >= -1.0 && x <= 1.0e6)) throw Error(LD_ERR_INVALID, message);
    const long long v = std::llrint(1000.0 * x);
    if (v < lo || v > hi) throw Error(LD_ERR_INVALID, message);
    return (int)v;
}

// The links grouped by a source anchor each.  D is symmetric, so either anchor of a link may be its source: the anchor that
// covers most links not yet covered (the smallest atom index among equals) becomes a source and takes them all, until none is
// left -- the greedy vertex cover, so that links which share an anchor share one field.
struct Grouping {
    std::vector<uint32_t> source, first, target, link;
};
Grouping group_links(size_t n_links, const uint32_t *links) {
    Grouping g;
    std::vector<char> covered(n_links, 0);
    size_t left = n_links;
    g.first.push_back(0);
    while (left) {
        std::map<uint32_t, uint32_t> degree;
        for (size_t l = 0; l < n_links; l++) {
            if (covered[l]) continue;
            degree[links[2 * l]]++;
            if (links[2 * l + 1] != links[2 * l]) degree[links[2 * l + 1]]++;
        }
        uint32_t best = 0, most = 0;
        for (const auto &d : degree)
            if (d.second > most) best = d.first, most = d.second;
        g.source.push_back(best);
        for (size_t l = 0; l < n_links; l++) {
            if (covered[l] || (links[2 * l] != best && links[2 * l + 1] != best)) continue;
            g.target.push_back(links[2 * l] == best ? links[2 * l + 1] : links[2 * l]);
            g.link.push_back((uint32_t)l);
            covered[l] = 1;
            left--;
        }
        g.first.push_back((uint32_t)g.link.size());
    }
    return g;
}

}  // namespace

void Complex::crosslinks(size_t n, const double *poses, size_t stride, size_t n_links, const uint32_t *links, double probe, double cell,
                         double reach, double max_length, uint64_t *straight2, uint32_t *path) {
    XlinkDevice d;
    d.probe = thousandths_in(probe, 0, kSasaMaxProbe, "probe must be 0 .. 2.0 A");
    d.h = thousandths_in(cell, kXlinkMinCell, kXlinkMaxCell, "cell must be 0.5 .. 2.0 A");
    d.reach = thousandths_in(reach, 1, kXlinkMaxReach, "reach must be 0.001 .. 6.0 A");
    d.M = thousandths_in(max_length, d.h, kXlinkMaxLength, "max_length must be cell .. 60.0 A");
    if (d.M / d.h > kXlinkMaxSteps) throw Error(LD_ERR_INVALID, "max_length must be 80 cells at most");
    if (n_links == 0 || n_links > (size_t)kXlinkMaxLinks) throw Error(LD_ERR_INVALID, "n_links must be 1 .. 4096");
    if (!links) throw Error(LD_ERR_INVALID, "null links");
    for (size_t k = 0; k < 2 * n_links; k++)
        if (links[k] >= n_atoms()) throw Error(LD_ERR_INVALID, "link " + std::to_string(k / 2) + " names an atom index beyond the complex");
    if (path && sasa_.n_part == 0) throw Error(LD_ERR_INVALID, "no atom takes part (all hydrogens or membrane beads)");
    d.w2 = (int)xlink_isqrt(2ll * d.h * d.h);
    d.w3 = (int)xlink_isqrt(3ll * d.h * d.h);
    d.rmax = 2 * (sasa_r_max_ + d.probe - 1) / d.h + 1;
    if ((long long)sasa_.n_part * d.rmax * d.rmax > (long long)INT_MAX) throw Error(LD_ERR_INVALID, "too many atoms for the rows of this cell");
    d.n_part = sasa_.n_part;
    d.part_atom = sasa_.part_atom;
    d.part_radius = sasa_.part_radius;
    d.n_links = (int)n_links;
    if (n == 0) return;
    check_poses(n, poses, stride);

    Grouping g;
    if (path) g = group_links(n_links, links);
    d.n_sources = (int)g.source.size();
    const size_t chunk = chunk_of(n_links * (sizeof(uint64_t) + sizeof(uint32_t)), n);
    const size_t per_slot = xlink_slot_bytes(d.n_part, d.M, d.h);
    const size_t slots = path ? chunk_of(per_slot, chunk * g.source.size(), kXlinkSlots) : 0;  // no search, no slot
    std::vector<uint64_t> h_straight(straight2 ? n * n_links : 0);
    std::vector<uint32_t> h_path(path ? n * n_links : 0);
    upload_poses(n, poses, stride);
    char *d_slots;
    unsigned long long *d_straight;
    uint32_t *d_path, *d_links, *d_source, *d_first, *d_target, *d_link;
    int *d_overflow;
    carve_into(d_ws_, [&](Carver &c) { d_slots = c.take<char>(slots * per_slot); });
    carve_into(d_ids_, [&](Carver &c) {
        d_straight = c.take<unsigned long long>(straight2 ? chunk * n_links : 0), d_path = c.take<uint32_t>(path ? chunk * n_links : 0);
        d_overflow = c.take<int>(1);
    });
    carve_into(d_xlink_, [&](Carver &c) {
        d_links = c.take<uint32_t>(2 * n_links);
        d_source = c.take<uint32_t>(g.source.size()), d_first = c.take<uint32_t>(g.first.size());  // all empty without a search
        d_target = c.take<uint32_t>(g.target.size()), d_link = c.take<uint32_t>(g.link.size());
    });
    auto upload = [&](uint32_t *to, const uint32_t *from, size_t count) {
        if (count) hip_check(hipMemcpyAsync(to, from, count * sizeof(uint32_t), hipMemcpyHostToDevice, stream_), "hipMemcpy H2D links");
    };
    upload(d_links, links, 2 * n_links);
    if (path) {
        upload(d_source, g.source.data(), g.source.size()), upload(d_first, g.first.data(), g.first.size());
        upload(d_target, g.target.data(), g.target.size()), upload(d_link, g.link.data(), g.link.size());
    }
    d.source = d_source, d.first = d_first, d.target = d_target, d.link = d_link;
    const double *d_poses = static_cast<const double *>(d_poses_.ptr);
    begin_timed(d_overflow);
    for (size_t i0 = 0; i0 < n; i0 += chunk) {
        const size_t m = std::min(chunk, n - i0);
        if (straight2) {
            hip_check(launch_xlink_straight(dev_, d_poses + i0 * stride, stride, m, d_links, d.n_links, d_straight, d_overflow, stream_),
                      "xlink_straight launch");
            hip_check(hipMemcpyAsync(h_straight.data() + i0 * n_links, d_straight, m * n_links * sizeof(uint64_t), hipMemcpyDeviceToHost, stream_),
                      "hipMemcpy D2H");
        }
        if (path) {
            hip_check(launch_xlink_paths(dev_, d, d_poses + i0 * stride, stride, m, std::min(slots, m * g.source.size()), d_slots, d_path,
                                         d_overflow, stream_),
                      "xlink_paths launch");
            hip_check(hipMemcpyAsync(h_path.data() + i0 * n_links, d_path, m * n_links * sizeof(uint32_t), hipMemcpyDeviceToHost, stream_),
                      "hipMemcpy D2H");
        }
    }
    // nothing reaches the caller before the overflow flags are known
    finish_timed(d_overflow, "complex_crosslinks", kXlinkOverflow);
    if (straight2) std::copy(h_straight.begin(), h_straight.end(), straight2);
    if (path) std::copy(h_path.begin(), h_path.end(), path);
}

}  // namespace ld
