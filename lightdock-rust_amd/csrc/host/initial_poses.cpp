#include "initial_poses.hpp"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "error.hpp"
#include "kernels/gso_step.hpp"

namespace ld {

namespace {

inline uint32_t rotl(uint32_t v, int n) { return (v << n) | (v >> (32 - n)); }

inline void quarter_round(uint32_t x[16], int a, int b, int c, int d) {
    x[a] += x[b]; x[d] ^= x[a]; x[d] = rotl(x[d], 16);
    x[c] += x[d]; x[b] ^= x[c]; x[b] = rotl(x[b], 12);
    x[a] += x[b]; x[d] ^= x[a]; x[d] = rotl(x[d], 8);
    x[c] += x[d]; x[b] ^= x[c]; x[b] = rotl(x[b], 7);
}

// The draws of one row: u64 number k of the stream is words 2 (k % 8), 2 (k % 8) + 1 of block k / 8.
class RowStream {
   public:
    RowStream(const uint32_t key[8], uint64_t base) : base_(base) { std::memcpy(key_, key, sizeof key_); }
    uint64_t bits() {
        if (used_ >> kPoseDrawShift) throw Error(LD_ERR_INTERNAL, "a pose row asked for more than 65536 draws");
        const uint64_t draw = base_ + used_++;
        if (!have_ || (draw >> 3) != block_no_) {
            block_no_ = draw >> 3;
            chacha20_block(key_, block_no_, block_);
            have_ = true;
        }
        const int w = (int)(draw & 7) * 2;
        return ((uint64_t)block_[w + 1] << 32) | block_[w];
    }
    double unit() { return (double)(bits() >> 11) * 0x1p-53; }   // u in [0, 1)
    double symmetric() { return 2.0 * unit() - 1.0; }           // v = 2 u - 1
    uint64_t used() const { return used_; }

   private:
    uint32_t key_[8];
    uint64_t base_, used_ = 0, block_no_ = 0;
    uint32_t block_[16];
    bool have_ = false;
};

inline double norm3(const double v[3]) { return std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }

size_t pick(RowStream &s, size_t n) {
    const size_t i = (size_t)std::floor(s.unit() * (double)n);
    return i < n ? i : n - 1;
}

// The shortest-arc rotation taking unit(l) to unit(d), (w, x, y, z); a zero vector on either side: the identity.
void arc_rotation(const double l[3], const double d[3], double q[4]) {
    const double nl = norm3(l), nd = norm3(d);
    q[0] = 1.0;
    q[1] = q[2] = q[3] = 0.0;
    if (!(nl > 0.0) || !(nd > 0.0)) return;
    const double a[3] = {l[0] / nl, l[1] / nl, l[2] / nl}, b[3] = {d[0] / nd, d[1] / nd, d[2] / nd};
    const double w = 1.0 + ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]);
    if (w < 1e-12) {   // antiparallel: half a turn about a x e, e the axis of a's smallest component
        int axis = 0;
        for (int c = 1; c < 3; c++)
            if (std::fabs(a[c]) < std::fabs(a[axis])) axis = c;
        double e[3] = {0.0, 0.0, 0.0};
        e[axis] = 1.0;
        const double c[3] = {a[1] * e[2] - a[2] * e[1], a[2] * e[0] - a[0] * e[2], a[0] * e[1] - a[1] * e[0]};
        const double nc = norm3(c);
        q[0] = 0.0;
        q[1] = c[0] / nc;
        q[2] = c[1] / nc;
        q[3] = c[2] / nc;
        return;
    }
    const double c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    const double nq = std::sqrt(((w * w + c[0] * c[0]) + c[1] * c[1]) + c[2] * c[2]);
    q[0] = w / nq;
    q[1] = c[0] / nq;
    q[2] = c[1] / nq;
    q[3] = c[2] / nq;
}

}  // namespace

void chacha20_block(const uint32_t key[8], uint64_t counter, uint32_t out[16]) {
    uint32_t s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u};
    for (int i = 0; i < 8; i++) s[4 + i] = key[i];
    s[12] = (uint32_t)counter;
    s[13] = (uint32_t)(counter >> 32);
    s[14] = s[15] = 0;
    uint32_t x[16];
    std::memcpy(x, s, sizeof x);
    for (int r = 0; r < 10; r++) {
        quarter_round(x, 0, 4, 8, 12); quarter_round(x, 1, 5, 9, 13); quarter_round(x, 2, 6, 10, 14); quarter_round(x, 3, 7, 11, 15);
        quarter_round(x, 0, 5, 10, 15); quarter_round(x, 1, 6, 11, 12); quarter_round(x, 2, 7, 8, 13); quarter_round(x, 3, 4, 9, 14);
    }
    for (int i = 0; i < 16; i++) out[i] = x[i] + s[i];
}

void initial_poses(const PoseRequest &r, double *rows, uint64_t *draws) {
    if (r.n == 0) return;
    if (!rows) throw Error(LD_ERR_INVALID, "null argument");
    if (r.glowworms < 1 || r.first >= r.glowworms || r.n > r.glowworms - r.first)
        throw Error(LD_ERR_INVALID, "rows first .. first + n - 1 must be glowworms of the run");
    if (r.glowworms > ((size_t)1 << 24) || r.swarm >= ((size_t)1 << 24)) throw Error(LD_ERR_INVALID, "at most 2^24 swarms and glowworms");
    if (r.anm_rec > 4096 || r.anm_lig > 4096) throw Error(LD_ERR_INVALID, "at most 4096 modes a side");
    if (!(r.radius >= 0.0) || !std::isfinite(r.radius)) throw Error(LD_ERR_INVALID, "radius must be finite and not negative");
    for (double c : r.centre)
        if (!std::isfinite(c)) throw Error(LD_ERR_INVALID, "non-finite centre");
    if ((r.n_rec && !r.rec_points) || (r.n_lig && !r.lig_points)) throw Error(LD_ERR_INVALID, "null restraint points");
    for (size_t i = 0; i < 3 * r.n_rec; i++)
        if (!std::isfinite(r.rec_points[i])) throw Error(LD_ERR_INVALID, "non-finite receptor restraint point");
    for (size_t i = 0; i < 3 * r.n_lig; i++)
        if (!std::isfinite(r.lig_points[i])) throw Error(LD_ERR_INVALID, "non-finite ligand restraint point");

    uint32_t key[8];
    stdrng_key_from_seed(r.seed, key);
    const size_t modes = r.anm_rec + r.anm_lig, len = 7 + modes;
    std::vector<double> out(r.n * len);
    std::vector<uint64_t> used(r.n);
    for (size_t k = 0; k < r.n; k++) {
        const uint64_t g = r.first + k;
        RowStream s(key, ((uint64_t)r.swarm * r.glowworms + g) << kPoseDrawShift);
        double *row = &out[k * len];
        // 1. the translation: a point of the unit ball by rejection
        double v[3];
        do {
            for (double &c : v) c = s.symmetric();
        } while (!((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2] <= 1.0));
        for (int c = 0; c < 3; c++) row[c] = r.centre[c] + r.radius * v[c];
        if (r.n_rec && r.n_lig) {
            // 3. a receptor restraint residue faces a ligand one
            const size_t ir = pick(s, r.n_rec), il = pick(s, r.n_lig);
            const double *p = r.rec_points + 3 * ir;
            const double d[3] = {p[0] - row[0], p[1] - row[1], p[2] - row[2]};
            arc_rotation(r.lig_points + 3 * il, d, row + 3);
        } else {
            // 2. a uniform rotation (Marsaglia)
            double x1, y1, r1, x2, y2, r2;
            do {
                x1 = s.symmetric();
                y1 = s.symmetric();
                r1 = x1 * x1 + y1 * y1;
            } while (!(r1 < 1.0));
            do {
                x2 = s.symmetric();
                y2 = s.symmetric();
                r2 = x2 * x2 + y2 * y2;
            } while (!(r2 < 1.0 && r2 > 0.0));
            const double scale = std::sqrt((1.0 - r1) / r2);
            row[3] = x1;
            row[4] = y1;
            row[5] = x2 * scale;
            row[6] = y2 * scale;
        }
        // 4. the mode extents: standard normals by the polar method, a left-over one discarded
        for (size_t m = 0; m < modes;) {
            double v1, v2, sq;
            do {
                v1 = s.symmetric();
                v2 = s.symmetric();
                sq = v1 * v1 + v2 * v2;
            } while (!(sq > 0.0 && sq < 1.0));
            const double f = std::sqrt((-2.0 * std::log(sq)) / sq);
            row[7 + m++] = v1 * f;
            if (m < modes) row[7 + m++] = v2 * f;
        }
        used[k] = s.used();
    }
    std::memcpy(rows, out.data(), out.size() * sizeof(double));
    if (draws) std::memcpy(draws, used.data(), used.size() * sizeof(uint64_t));
}

}  // namespace ld
