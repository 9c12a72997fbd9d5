// assess.hpp -- launch interface of K3d, model quality against a reference complex (kernels/assess.hip; DESIGN §5 K3d;
// lightdock_hip.h, "Model quality"): what the host side (complex.cpp) and the kernels share, and the f64 arithmetic that
// follows the integer sums (assess_solve_pose), which is host code too so that a CPU build can check it.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "kernels/cluster.hpp"

namespace ld {

constexpr int kAssessThreads = 512;
constexpr int kAssessSlots = 1024;           // as kContactSlots
constexpr int kAssessBound = 2000000;        // thousandths: a used atom's posed coordinate is within +-2000 A, below 2^21
constexpr size_t kAssessMaxUsed = size_t(1) << 20;
constexpr size_t kAssessChunkPoses = 65536;  // poses a launch pair: 20 MiB of sums

// The sums of one fit set: sum m (3), sum |m|^2 (1, an unsigned word), sum m_a r_b (9, row a of the model, column b of the
// reference).  m: the model's thousandths; r: the reference's, centred (AssessDevice::used_ref).
constexpr int kAssessSetWords = 13;
// A pose's words: the receptor's fit atoms, the ligand's fit atoms, the interface fit atoms of both sides, kept.
constexpr int kAssessRec = 0, kAssessLig = 13, kAssessInt = 26, kAssessKept = 39, kAssessWords = 40;

struct AssessDevice {
    int n_used = 0, n_used_rec = 0, n_native = 0;  // used atoms, the receptor's first
    const uint32_t *used_atom = nullptr;  // n_used complex atom indices, ascending
    // n_used: the matched reference record's centred thousandths (x, y, z); w: bit 0 fit atom, bit 1 interface fit atom
    const int4 *used_ref = nullptr;
    // n_native, sorted by (receptor residue, ligand residue): the used atoms [x, y) of the receptor residue and [z, w) of
    // the ligand residue
    const int4 *native = nullptr;
};

// What the reference contributes to a pose's superpositions, fixed at ld_complex_set_reference.
struct AssessSolve {
    long long n_rec = 0, n_lig = 0, n_int = 0;     // fit atoms of each set
    long long sr_rec[3] = {}, sr_lig[3] = {}, sr_int[3] = {};  // sum r of each set
    double g_rec = 0, g_int = 0;  // sum |r - mean r|^2 of the set
    double g_lig = 0;             // sum |r - mean r of the RECEPTOR's fit atoms|^2 over the ligand's fit atoms
};

// Every launch reads `m` as ComplexDevice says and pose rows of 7 + m.anm_rec + m.anm_lig doubles, `stride` doubles apart.

// `slots` workgroups, 1 .. kAssessSlots.  poses: n rows; d: as AssessDevice says; atoms_ws: slots x d.n_used int4;
// sums: n x kAssessWords; overflow: one int, set when a used atom's coordinate is beyond +-kAssessBound.
hipError_t launch_complex_assess_sums(const ComplexDevice &m, const AssessDevice &d, const double *poses, size_t stride, size_t n,
                                      uint32_t C2, size_t slots, int4 *atoms_ws, long long *sums, int *overflow,
                                      hipStream_t stream);
// A thread a pose.  sums: n x kAssessWords, as complex_assess_sums left them; kept, lrmsd, irmsd: n each.
hipError_t launch_complex_assess_solve(const AssessSolve &k, const long long *sums, size_t n, uint32_t *kept, double *lrmsd,
                                       double *irmsd, hipStream_t stream);

// --- after the sums: f64 from exact operands --------------------------------------------------------------------------

typedef __int128 assess_wide;

#ifdef __clang__  // the device compiler keeps the small matrices in registers only when their loops are unrolled
#define LD_ASSESS_UNROLL _Pragma("unroll")
#define LD_ASSESS_NO_UNROLL _Pragma("unroll 1")
#else
#define LD_ASSESS_UNROLL
#define LD_ASSESS_NO_UNROLL
#endif

// Two roundings at most: both halves are exact or rounded once, their sum is rounded once.
__host__ __device__ inline double assess_to_double(assess_wide v) {
    const bool negative = v < 0;
    const unsigned __int128 u = negative ? (unsigned __int128)0 - (unsigned __int128)v : (unsigned __int128)v;
    const double d = (double)(uint64_t)(u >> 64) * 18446744073709551616.0 + (double)(uint64_t)u;
    return negative ? -d : d;
}

// Horn's closed form on the 3 x 3 S[a][b] = sum (m_a - mean)(r_b - mean): the unit quaternion (w, x, y, z) of the proper
// rotation R that maximises sum r . (R m), and that maximum, the largest eigenvalue of the symmetric 4 x 4.  Cyclic Jacobi,
// a fixed number of sweeps; no case is special (a zero off-diagonal element is simply not rotated).  The eigenvalue is the
// Rayleigh quotient of the ORIGINAL matrix at the eigenvector found, so the sweeps' rounding does not add up in it.
constexpr int kAssessSweeps = 10;

__host__ __device__ inline double assess_horn(const double S[3][3], double q[4]) {
    const double N[4][4] = {
        {S[0][0] + S[1][1] + S[2][2], S[1][2] - S[2][1], S[2][0] - S[0][2], S[0][1] - S[1][0]},
        {S[1][2] - S[2][1], S[0][0] - S[1][1] - S[2][2], S[0][1] + S[1][0], S[2][0] + S[0][2]},
        {S[2][0] - S[0][2], S[0][1] + S[1][0], -S[0][0] + S[1][1] - S[2][2], S[1][2] + S[2][1]},
        {S[0][1] - S[1][0], S[2][0] + S[0][2], S[1][2] + S[2][1], -S[0][0] - S[1][1] + S[2][2]}};
    double a[4][4], v[4][4];
    LD_ASSESS_UNROLL
    for (int i = 0; i < 4; i++)
        LD_ASSESS_UNROLL
        for (int j = 0; j < 4; j++) {
            a[i][j] = N[i][j];
            v[i][j] = i == j ? 1.0 : 0.0;
        }
    LD_ASSESS_NO_UNROLL
    for (int sweep = 0; sweep < kAssessSweeps; sweep++) {
        LD_ASSESS_UNROLL
        for (int p = 0; p < 3; p++)
            LD_ASSESS_UNROLL
            for (int r = p + 1; r < 4; r++) {
                const double apr = a[p][r];
                if (apr == 0.0) continue;
                const double theta = (a[r][r] - a[p][p]) / (2.0 * apr);  // +-inf for a tiny element: t = 0
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                a[p][p] -= t * apr;
                a[r][r] += t * apr;
                a[p][r] = a[r][p] = 0.0;
                LD_ASSESS_UNROLL
                for (int k = 0; k < 4; k++) {
                    if (k != p && k != r) {
                        const double akp = a[k][p], akr = a[k][r];
                        a[k][p] = a[p][k] = c * akp - s * akr;
                        a[k][r] = a[r][k] = s * akp + c * akr;
                    }
                    const double vkp = v[k][p], vkr = v[k][r];
                    v[k][p] = c * vkp - s * vkr;
                    v[k][r] = s * vkp + c * vkr;
                }
            }
    }
    int best = 0;
    double largest = a[0][0];
    LD_ASSESS_UNROLL
    for (int k = 1; k < 4; k++)
        if (a[k][k] > largest) {
            largest = a[k][k];
            best = k;
        }
    double e[4];
    LD_ASSESS_UNROLL
    for (int k = 0; k < 4; k++) e[k] = best == 0 ? v[k][0] : best == 1 ? v[k][1] : best == 2 ? v[k][2] : v[k][3];
    const double norm = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2] + e[3] * e[3]);  // 1 to rounding: V is a product of rotations
    LD_ASSESS_UNROLL
    for (int k = 0; k < 4; k++) q[k] = e[k] / norm;
    double lambda = 0.0;
    LD_ASSESS_UNROLL
    for (int i = 0; i < 4; i++) {
        double row = 0.0;
        LD_ASSESS_UNROLL
        for (int j = 0; j < 4; j++) row += N[i][j] * q[j];
        lambda += q[i] * row;
    }
    return lambda;
}

// One set's own superposition: sum |m - mean|^2 and S = sum (m - mean)(r - mean)^T from the exact n sum|m|^2 - |sum m|^2
// and n sum m r^T - (sum m)(sum r)^T; returns max(0, (G_model + G_ref - 2 lambda) / n) in thousandths^2 and the quaternion.
__host__ __device__ inline double assess_fit(const long long *w, long long n, const long long sr[3], double g_ref, double q[4]) {
    const assess_wide nn = n;
    const assess_wide sm2 = (assess_wide)w[0] * w[0] + (assess_wide)w[1] * w[1] + (assess_wide)w[2] * w[2];
    const double dn = (double)n;
    const double g_model = assess_to_double(nn * (assess_wide)(unsigned long long)w[3] - sm2) / dn;
    double S[3][3];
    LD_ASSESS_UNROLL
    for (int a = 0; a < 3; a++)
        LD_ASSESS_UNROLL
        for (int b = 0; b < 3; b++) S[a][b] = assess_to_double(nn * w[4 + 3 * a + b] - (assess_wide)w[a] * sr[b]) / dn;
    const double lambda = assess_horn(S, q);
    return fmax(0.0, ((g_model + g_ref) - 2.0 * lambda) / dn);
}

// The words of one pose -> L-RMSD and i-RMSD in A.  Never NaN: every operand is a finite integer, fmax drops a negative
// rounding residue, and the eigensolver divides by nothing that can vanish.
__host__ __device__ inline void assess_solve_pose(const AssessSolve &k, const long long *w, double *lrmsd, double *irmsd) {
    double q[4];
    *irmsd = sqrt(assess_fit(w + kAssessInt, k.n_int, k.sr_int, k.g_int, q)) / 1000.0;
    (void)assess_fit(w + kAssessRec, k.n_rec, k.sr_rec, k.g_rec, q);
    const double R[3][3] = {
        {q[0] * q[0] + q[1] * q[1] - q[2] * q[2] - q[3] * q[3], 2.0 * (q[1] * q[2] - q[0] * q[3]), 2.0 * (q[1] * q[3] + q[0] * q[2])},
        {2.0 * (q[1] * q[2] + q[0] * q[3]), q[0] * q[0] - q[1] * q[1] + q[2] * q[2] - q[3] * q[3], 2.0 * (q[2] * q[3] - q[0] * q[1])},
        {2.0 * (q[1] * q[3] - q[0] * q[2]), 2.0 * (q[2] * q[3] + q[0] * q[1]), q[0] * q[0] - q[1] * q[1] - q[2] * q[2] + q[3] * q[3]}};
    // the ligand's fit atoms about the RECEPTOR's centroids (sum m_R / n_R, sum r_R / n_R), times n_R^2, exactly:
    //   G = n_R^2 sum|m|^2 - 2 n_R (sum m_R . sum m_L) + n_L |sum m_R|^2
    //   C = n_R^2 sum m r^T - n_R (sum m_R)(sum r_L)^T - n_R (sum m_L)(sum r_R)^T + n_L (sum m_R)(sum r_R)^T
    // (each term below 2^105 with at most 2^20 atoms within 2^21 thousandths)
    const long long *r = w + kAssessRec, *l = w + kAssessLig;
    const assess_wide nr = k.n_rec, nl = k.n_lig;
    const double nr2 = (double)k.n_rec * (double)k.n_rec;
    const assess_wide dot = (assess_wide)r[0] * l[0] + (assess_wide)r[1] * l[1] + (assess_wide)r[2] * l[2];
    const assess_wide rr = (assess_wide)r[0] * r[0] + (assess_wide)r[1] * r[1] + (assess_wide)r[2] * r[2];
    const double g_model = assess_to_double(nr * nr * (assess_wide)(unsigned long long)l[3] - 2 * nr * dot + nl * rr) / nr2;
    double trace = 0.0;
    LD_ASSESS_UNROLL
    for (int b = 0; b < 3; b++)
        LD_ASSESS_UNROLL
        for (int a = 0; a < 3; a++) {
            const assess_wide c = nr * nr * l[4 + 3 * a + b] - nr * ((assess_wide)r[a] * k.sr_lig[b]) -
                                  nr * ((assess_wide)l[a] * k.sr_rec[b]) + nl * ((assess_wide)r[a] * k.sr_rec[b]);
            trace += R[b][a] * (assess_to_double(c) / nr2);
        }
    *lrmsd = sqrt(fmax(0.0, ((g_model + k.g_lig) - 2.0 * trace) / (double)k.n_lig)) / 1000.0;
}

}  // namespace ld
