// ccs.cpp -- the host side of the collision cross-section (lightdock_hip.h, "Collision cross-section"):
// Complex::ccs -- the argument checks, the selection, the rigid receptor's atoms and the layout of its 64 bitmaps, the
// chunking (chunk_of), the workspace (every block laid out through device_memory.hpp's Carver) and the launches of
// kernels/ccs.hpp.
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "complex.hpp"
#include "kernels/ccs.hpp"
#include "kernels/complex_rule.hpp"

namespace ld {

namespace {

const char *const kCcsOverflow = "a posed coordinate is beyond +-1.0e6 A, or a view's box holds more than 2^28 lattice points";

}  // namespace

void Complex::ccs(size_t n, const double *poses, size_t stride, int what, double probe, double cell, uint32_t *counts, uint64_t *sums) {
    if (!(probe >= 0.0 && probe <= 2.0)) throw Error(LD_ERR_INVALID, "probe must be 0 .. 2.0 A");
    if (!(cell > 0.0 && cell < 1.0e6)) throw Error(LD_ERR_INVALID, "cell must be 0.1 .. 2.0 A");  // the rule is on h, below
    if (what < 0 || what > 2) throw Error(LD_ERR_INVALID, "what must be 0 (receptor), 1 (ligand) or 2 (complex)");
    CcsDevice d;
    d.probe = (int)std::llrint(1000.0 * probe);
    d.h = (int)std::llrint(1000.0 * cell);
    if (d.h < kCcsMinCell || d.h > kCcsMaxCell) throw Error(LD_ERR_INVALID, "cell must be 0.1 .. 2.0 A");
    d.first = what == 1 ? sasa_.n_part_rec : 0;
    d.count = (what == 0 ? sasa_.n_part_rec : sasa_.n_part) - d.first;
    if (d.count == 0) throw Error(LD_ERR_INVALID, "no selected atom takes part (all hydrogens or membrane beads)");
    d.rmax = 2 * (sasa_r_max_ + d.probe) / d.h + 1;
    if ((long long)sasa_.n_part * d.rmax > (long long)INT_MAX) throw Error(LD_ERR_INVALID, "too many atoms for the rows of this cell");
    d.part_atom = sasa_.part_atom;
    d.part_radius = sasa_.part_radius;
    if (n == 0) return;
    check_poses(n, poses, stride);

    // without receptor modes the receptor's discs are the same for every pose: its atoms and the boxes of its 64 views
    // are made here, its bitmaps once a call on the device -- if they fit kCcsRigidBytes; else every pose rasterises it
    std::vector<int4> rec_atoms;
    std::vector<CcsRecView> rec_views;
    size_t rec_words = 0;
    bool rigid = what == 2 && dev_.anm_rec == 0 && sasa_.n_part_rec >= 1 && sasa_.n_part > sasa_.n_part_rec;
    if (rigid) {
        rec_atoms.reserve((size_t)sasa_.n_part_rec);
        for (size_t a = 0; a < sasa_radius_[0].size(); a++) {
            if (sasa_radius_[0][a] == 0) continue;
            int v[3];
            for (int k = 0; k < 3; k++) {
                const double c = thousandths(rec_.xyz[3 * a + k]);  // an unposed atom: the rounding alone
                if (!(std::fabs(c) <= (double)kComplexCoordBound)) throw Error(LD_ERR_INVALID, kCcsOverflow);
                v[k] = (int)c;
            }
            rec_atoms.push_back(make_int4(v[0], v[1], v[2], (int)sasa_radius_[0][a] + d.probe));
        }
        rec_views.resize(kCcsViews);
        for (int v = 0; v < kCcsViews && rigid; v++) {
            CcsRecView &w = rec_views[v];
            w.lo_a = w.lo_b = INT_MAX, w.hi_a = w.hi_b = INT_MIN;
            for (const int4 &p : rec_atoms) {
                const int a = ccs_project(kCcsFrames[v], p.x, p.y, p.z), b = ccs_project(kCcsFrames[v] + 3, p.x, p.y, p.z);
                w.lo_a = std::min(w.lo_a, a - p.w), w.hi_a = std::max(w.hi_a, a + p.w);
                w.lo_b = std::min(w.lo_b, b - p.w), w.hi_b = std::max(w.hi_b, b + p.w);
            }
            const CcsBox box = ccs_box(w.lo_a, w.hi_a, w.lo_b, w.hi_b, d.h);
            w.wc0 = box.wc0(), w.j0 = box.j0, w.pitch = box.wc1() - box.wc0() + 1, w.rows = (int)box.rows();
            w.offset = rec_words;
            // a receptor box beyond the bound is every pose's: the plain form finds and refuses it
            if (box.columns() * box.rows() > kCcsMaxBox) rigid = false;
            rec_words += (size_t)w.pitch * (size_t)w.rows;
            if (rec_words * sizeof(uint32_t) > kCcsRigidBytes) rigid = false;
        }
    }
    if (rigid) d.first = sasa_.n_part_rec, d.count = sasa_.n_part - sasa_.n_part_rec;

    const size_t per_slot = ccs_slot_bytes(d.count);
    const size_t slots = chunk_of(per_slot, n, kCcsSlots);
    const size_t chunk = chunk_of(kCcsViews * sizeof(uint32_t) + sizeof(unsigned long long), n);
    std::vector<uint32_t> h_counts(n * kCcsViews);
    std::vector<uint64_t> h_sums(n);
    upload_poses(n, poses, stride);
    int4 *d_slots, *d_rec_atoms;
    CcsRecView *d_rec_views;
    uint32_t *d_rec_bits, *d_counts;
    unsigned long long *d_sums;
    int *d_overflow;
    carve_into(d_ws_, [&](Carver &c) { d_slots = c.take<int4>(slots * 2 * (size_t)d.count); });
    carve_into(d_ids_, [&](Carver &c) {
        d_counts = c.take<uint32_t>(chunk * kCcsViews), d_sums = c.take<unsigned long long>(chunk), d_overflow = c.take<int>(1);
    });
    // what only the rigid-receptor form needs has no elements, and so is null, without it
    carve_into(d_ccs_, [&](Carver &c) {
        d_rec_atoms = c.take<int4>(rigid ? rec_atoms.size() : 0), d_rec_views = c.take<CcsRecView>(rigid ? rec_views.size() : 0);
        d_rec_bits = c.take<uint32_t>(rigid ? rec_words : 0);
    });
    if (rigid) {
        hip_check(hipMemcpyAsync(d_rec_atoms, rec_atoms.data(), rec_atoms.size() * sizeof(int4), hipMemcpyHostToDevice, stream_), "hipMemcpy H2D atoms");
        hip_check(hipMemcpyAsync(d_rec_views, rec_views.data(), rec_views.size() * sizeof(CcsRecView), hipMemcpyHostToDevice, stream_), "hipMemcpy H2D views");
    }
    const double *d_poses = static_cast<const double *>(d_poses_.ptr);
    begin_timed(d_overflow);
    if (rigid) {
        hip_check(hipMemsetAsync(d_rec_bits, 0, rec_words * sizeof(uint32_t), stream_), "hipMemset");
        hip_check(launch_ccs_receptor(d_rec_atoms, (int)rec_atoms.size(), d.h, d.rmax, d_rec_views, d_rec_bits, stream_), "ccs_receptor launch");
        d.rec_views = d_rec_views;
        d.rec_bits = d_rec_bits;
    }
    for (size_t i0 = 0; i0 < n; i0 += chunk) {
        const size_t m = std::min(chunk, n - i0);
        hip_check(launch_complex_ccs(dev_, d, d_poses + i0 * stride, stride, m, std::min(slots, m), d_slots, d_counts, d_sums, d_overflow, stream_),
                  "complex_ccs launch");
        hip_check(hipMemcpyAsync(h_counts.data() + i0 * kCcsViews, d_counts, m * kCcsViews * sizeof(uint32_t), hipMemcpyDeviceToHost, stream_), "hipMemcpy D2H");
        hip_check(hipMemcpyAsync(h_sums.data() + i0, d_sums, m * sizeof(uint64_t), hipMemcpyDeviceToHost, stream_), "hipMemcpy D2H");
    }
    // nothing reaches the caller before the overflow flags are known
    finish_timed(d_overflow, "complex_ccs", kCcsOverflow);
    if (counts) std::copy(h_counts.begin(), h_counts.end(), counts);
    if (sums) std::copy(h_sums.begin(), h_sums.end(), sums);
}

}  // namespace ld
