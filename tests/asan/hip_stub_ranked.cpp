// hip_stub_ranked.cpp -- TEST INFRASTRUCTURE for the sanitizer build of the host side (`make asan`, `make asan-assess`,
// `make asan-ranked`): the launches of kernels/ranked.hpp, beside tests/asan/hip_stub.cpp which stands in for the HIP
// runtime and every other kernel.  Device memory is host memory there, so ASan checks every extent below against what
// complex.cpp allocated.  Unlike the other stubs these DO what their kernels do, in plain C++, so that the host's round
// loop really runs and ends on them and ld_complex_cluster_ranked's outputs can be checked (tests/asan/ranked_check.cpp);
// each also touches both ends of every buffer its kernel reads or writes, the extents as ranked.hip indexes them.
#include <cfloat>
#include <cstring>

#include "kernels/ranked.hpp"
#include "ranked_host.hpp"
#include "stub_access.hpp"

namespace ld {

static bool sane(const RankedLaunch &r) { return r.n >= 1 && r.n_walk >= 1 && r.state && r.reps && r.status; }

hipError_t launch_ranked_begin(const RankedLaunch &r, double cutoff, double n_atoms, hipStream_t) {
    if (!sane(r) || !(n_atoms >= 1.0) || cutoff != cutoff) return hipErrorInvalidValue;
    for (int p = 0; p < r.n; p++) r.state[p] = -1;
    double s_max = -1.0;
    if (ranked_host::within_cutoff(0.0, n_atoms, cutoff)) {
        uint64_t lo = 0, hi;
        const double top = DBL_MAX;
        std::memcpy(&hi, &top, sizeof hi);
        if (ranked_host::within_cutoff(top, n_atoms, cutoff)) lo = hi;
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            double s;
            std::memcpy(&s, &mid, sizeof s);
            (ranked_host::within_cutoff(s, n_atoms, cutoff) ? lo : hi) = mid;
        }
        std::memcpy(&s_max, &lo, sizeof s_max);
    }
    std::memset(r.status, 0, sizeof *r.status);
    r.status->s_max = s_max;
    return hipSuccess;
}

hipError_t launch_ranked_pose(const ComplexDevice &m, const double *poses, size_t stride, int n, const uint32_t *walk, int n_walk,
                              int32_t *ws, RankedStatus *status, hipStream_t) {
    if (n < 1 || n_walk < 1) return hipErrorInvalidValue;
    peek_complex(m, poses, stride, (size_t)n);
    peek(walk, (size_t)n_walk);
    peek(ws, (size_t)n_walk * 3 * n);
    for (int a = 0; a < n_walk; a++) {
        if (walk[a] >= (uint32_t)(m.n_rec + m.n_lig)) return hipErrorInvalidValue;
        for (int p = 0; p < n; p++) {
            double v[3];
            ranked_host::pose_atom(m, poses + (size_t)p * stride, walk[a], v);
            for (int k = 0; k < 3; k++) {
                const double c = ranked_host::thousandths(v[k]);
                if (!(std::fabs(c) <= 2147483647.0)) status->overflow = 1;
                ws[((size_t)a * 3 + k) * n + p] = (int32_t)std::fmax(-2147483647.0, std::fmin(2147483647.0, c));
            }
        }
    }
    return hipSuccess;
}

// The sum of squared differences of two positions, with the early exit every kRankedGranule atoms.
static bool near(const RankedLaunch &r, const int32_t *ws, int p, int q) {
    double s = 0.0;
    for (int a0 = 0; a0 < r.n_walk; a0 += kRankedGranule) {
        const int a1 = a0 + kRankedGranule < r.n_walk ? a0 + kRankedGranule : r.n_walk;
        for (int row = 3 * a0; row < 3 * a1; row++) {
            const double d = (double)ws[(size_t)row * r.n + p] - (double)ws[(size_t)row * r.n + q];
            s += d * d;
        }
        if (!(s <= r.status->s_max)) return false;
    }
    return true;
}

hipError_t launch_ranked_pick(const RankedLaunch &r, const int32_t *ws, hipStream_t) {
    if (!sane(r)) return hipErrorInvalidValue;
    peek(ws, (size_t)r.n_walk * 3 * r.n);
    peek(r.state, (size_t)r.n);
    peek(r.reps, (size_t)r.n);
    RankedStatus *st = r.status;
    if (st->cursor < 0 || st->cursor > r.n || st->n_clusters < 0 || st->n_clusters > st->cursor) return hipErrorInvalidValue;
    int cand[kRankedBlock], lid[kRankedBlock], nc = 0;
    for (int p = st->cursor; p < r.n && nc < kRankedBlock; p++)
        if (r.state[p] == -1) cand[nc++] = p;
    unsigned long long leaders = 0;
    int count = 0;
    const int first = st->n_clusters;
    for (int k = 0; k < nc; k++) {
        unsigned long long m = 0;
        for (int j = 0; j < k; j++)
            if (near(r, ws, cand[j], cand[k])) m |= 1ull << j;
        m &= leaders;
        if (m == 0) {
            leaders |= 1ull << k;
            lid[k] = count;
            st->leaders[count] = cand[k];
            r.reps[first + count] = cand[k];
            r.state[cand[k]] = first + count;
            count++;
        } else {
            r.state[cand[k]] = first + lid[__builtin_ctzll(m)];
        }
    }
    st->n_clusters = first + count;
    st->n_leaders = count;
    st->n_candidates = nc;
    st->cursor = nc ? cand[nc - 1] + 1 : r.n;
    st->rounds += nc ? 1 : 0;
    return hipSuccess;
}

hipError_t launch_ranked_sweep(const RankedLaunch &r, const int32_t *ws, int from, hipStream_t) {
    if (!sane(r) || from < 0) return hipErrorInvalidValue;
    const RankedStatus *st = r.status;
    if (from > st->cursor) return hipErrorInvalidValue;   // `from` is a lower bound of the cursor: nothing behind it is skipped
    peek(ws, (size_t)r.n_walk * 3 * r.n);
    peek(r.state, (size_t)r.n);
    for (int p = st->cursor; p < r.n; p++) {
        if (r.state[p] != -1) continue;
        for (int l = 0; l < st->n_leaders; l++)
            if (near(r, ws, p, st->leaders[l])) {
                r.state[p] = st->n_clusters - st->n_leaders + l;
                break;
            }
    }
    return hipSuccess;
}

}  // namespace ld
