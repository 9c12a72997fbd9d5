// saxs.cpp -- the host side of the SAXS profiles (lightdock_hip.h, "Small-angle scattering"): the classes
// of a complex's atoms, the tables made with libm, argument checks, chunking (chunk_of), the workspace (every block laid out
// through device_memory.hpp's Carver) and the launch sequences of kernels/saxs.hpp, for a complex
// (Complex::distance_histogram, Complex::saxs) and for counts the caller gives (saxs_debye_host), and the fit.
#include "saxs.hpp"

#include <algorithm>
#include <cmath>
#include <string>

#include "complex.hpp"

namespace ld {

namespace {

constexpr double kFourPi = 4.0 * 3.14159265358979323846;
constexpr double kRho0 = 0.334;  // electrons / A^3 of the solvent

// Cromer-Mann a1..a4, b1..b4, c and the displaced volume V (A^3) of H, C, N, O, P, S: the rule's table.
const struct {
    double a[4], b[4], c, V;
} kFormFactor[kSaxsClasses] = {
    {{0.489918, 0.262003, 0.196767, 0.049879}, {20.6593, 7.74039, 49.5519, 2.20159}, 0.001305, 5.15},
    {{2.31000, 1.02000, 1.58860, 0.865000}, {20.8439, 10.2075, 0.568700, 51.6512}, 0.215600, 16.44},
    {{12.2126, 3.13220, 2.01250, 1.16630}, {0.005700, 9.89330, 28.9975, 0.582600}, -11.529, 2.49},
    {{3.04850, 2.28680, 1.54630, 0.867000}, {13.2771, 5.70110, 0.323900, 32.9089}, 0.250800, 9.13},
    {{6.43450, 4.17910, 1.78000, 1.49080}, {1.90670, 27.1570, 0.526000, 68.1645}, 1.11490, 5.73},
    {{6.90530, 5.20340, 1.43790, 1.58630}, {1.46790, 22.2151, 0.253600, 56.1720}, 0.866900, 19.86},
};

double form_factor(int e, double q) {
    const auto &t = kFormFactor[e];
    const double s = q / kFourPi, u = s * s;
    double f = 0.0;
    for (int k = 0; k < 4; k++) f = f + t.a[k] * std::exp(-t.b[k] * u);
    f = f + t.c;
    return f - kRho0 * t.V * std::exp(-(q * q) * std::pow(t.V, 2.0 / 3.0) / kFourPi);
}

void check_grid(uint32_t width, size_t bins) {
    if (width < (uint32_t)kSaxsMinWidth || width > (uint32_t)kSaxsMaxWidth) throw Error(LD_ERR_INVALID, "width must be 100 .. 2000 thousandths");
    if (bins < 1 || bins > (size_t)kSaxsMaxBins) throw Error(LD_ERR_INVALID, "bins must be 1 .. 1024");
}

void check_q(const double *q, size_t n_q) {
    if (n_q < 1 || n_q > (size_t)kSaxsMaxQ) throw Error(LD_ERR_INVALID, "n_q must be 1 .. 1024");
    if (!q) throw Error(LD_ERR_INVALID, "null q");
    for (size_t j = 0; j < n_q; j++)
        if (!(q[j] >= 0.0 && q[j] <= 1.0)) throw Error(LD_ERR_INVALID, "q " + std::to_string(j) + " is outside 0 .. 1.0 / A");
}

double sinc_at(double q, size_t k, uint32_t width) {
    const double r = ((double)k + 0.5) * (double)width / 1000.0, x = q * r;
    return x == 0.0 ? 1.0 : std::sin(x) / x;
}

// The tables behind a Debye launch, in the block the carver walks.
struct DeviceTables {
    double *sinc_t = nullptr, *self = nullptr, *cross = nullptr;
};

DeviceTables take_tables(const SaxsTables &t, Carver &c) {
    DeviceTables d;
    d.sinc_t = c.take<double>(t.sinc_t.size()), d.self = c.take<double>(t.self.size()), d.cross = c.take<double>(t.cross.size());
    return d;
}

void upload_tables(const SaxsTables &t, const DeviceTables &d, hipStream_t stream) {
    hip_check(hipMemcpyAsync(d.sinc_t, t.sinc_t.data(), t.sinc_t.size() * sizeof(double), hipMemcpyHostToDevice, stream), "hipMemcpy H2D sinc");
    hip_check(hipMemcpyAsync(d.self, t.self.data(), t.self.size() * sizeof(double), hipMemcpyHostToDevice, stream), "hipMemcpy H2D");
    hip_check(hipMemcpyAsync(d.cross, t.cross.data(), t.cross.size() * sizeof(double), hipMemcpyHostToDevice, stream), "hipMemcpy H2D");
}

}  // namespace

uint8_t saxs_class(const char *line, size_t len) {
    static const char *const element_of[kSaxsClasses] = {"H", "C", "N", "O", "P", "S"};
    if (record_residue_name(line) == "MMB") return (uint8_t)kSaxsNoPart;
    const std::string element = record_element(line, len);
    if (element == "D") return 0;
    for (int e = 0; e < kSaxsClasses; e++)
        if (element == element_of[e]) return (uint8_t)e;
    return (uint8_t)kSaxsNoPart;
}

void saxs_form_factors(const double *q, size_t n_q, double *f_out) {
    check_q(q, n_q);
    if (!f_out) throw Error(LD_ERR_INVALID, "null argument");
    for (size_t j = 0; j < n_q; j++)
        for (int e = 0; e < kSaxsClasses; e++) f_out[j * kSaxsClasses + e] = form_factor(e, q[j]);
}

void saxs_sinc(const double *q, size_t n_q, uint32_t width, size_t bins, double *s_out) {
    check_grid(width, bins);
    check_q(q, n_q);
    if (!s_out) throw Error(LD_ERR_INVALID, "null argument");
    for (size_t j = 0; j < n_q; j++)
        for (size_t k = 0; k < bins; k++) s_out[j * bins + k] = sinc_at(q[j], k, width);
}

SaxsTables saxs_tables(const double *q, size_t n_q, uint32_t width, size_t bins, const uint32_t *class_atoms) {
    SaxsTables t;
    t.sinc_t.resize(bins * n_q);
    t.self.resize(n_q);
    t.cross.resize(n_q * kSaxsPairClasses);
    for (size_t j = 0; j < n_q; j++) {
        for (size_t k = 0; k < bins; k++) t.sinc_t[k * n_q + j] = sinc_at(q[j], k, width);
        double f[kSaxsClasses], S = 0.0;
        for (int e = 0; e < kSaxsClasses; e++) {
            f[e] = form_factor(e, q[j]);
            S = S + (double)class_atoms[e] * (f[e] * f[e]);
        }
        t.self[j] = S;
        for (int e = 0; e < kSaxsClasses; e++)
            for (int g = e; g < kSaxsClasses; g++) t.cross[j * kSaxsPairClasses + saxs_pair_class((uint32_t)e, (uint32_t)g)] = (2.0 * f[e]) * f[g];
    }
    return t;
}

void saxs_debye_host(size_t n, const uint32_t *counts, uint32_t width, size_t bins, const uint32_t *class_atoms, const double *q,
                     size_t n_q, double *intensity) {
    check_grid(width, bins);
    check_q(q, n_q);
    if (!class_atoms) throw Error(LD_ERR_INVALID, "null class_atoms");
    if (n == 0) return;
    if (!counts || !intensity) throw Error(LD_ERR_INVALID, "null argument");
    const SaxsTables t = saxs_tables(q, n_q, width, bins, class_atoms);
    const size_t row_words = (size_t)kSaxsPairClasses * bins, row_bytes = row_words * sizeof(uint32_t);
    const size_t chunk = chunk_of(row_bytes, n);
    DeviceBuffer d_counts, d_rest;
    reserve_exact(d_counts, chunk * row_bytes);
    DeviceTables tables;
    double *d_intensity;
    carve_into(d_rest, [&](Carver &c) { tables = take_tables(t, c), d_intensity = c.take<double>(n * n_q); });
    upload_tables(t, tables, nullptr);
    SaxsDebye d;
    d.bins = (int)bins;
    d.n_q = (int)n_q;
    d.counts = static_cast<const uint32_t *>(d_counts.ptr);
    d.sinc_t = tables.sinc_t, d.self = tables.self, d.cross = tables.cross;
    for (size_t i0 = 0; i0 < n; i0 += chunk) {
        const size_t m = std::min(chunk, n - i0);
        hip_check(hipMemcpyAsync(d_counts.ptr, counts + i0 * row_words, m * row_bytes, hipMemcpyHostToDevice, nullptr), "hipMemcpy H2D counts");
        d.intensity = d_intensity + i0 * n_q;
        hip_check(launch_saxs_debye(d, m, nullptr), "saxs_debye launch");
    }
    std::vector<double> result(n * n_q);
    hip_check(hipMemcpyAsync(result.data(), d_intensity, n * n_q * sizeof(double), hipMemcpyDeviceToHost, nullptr), "hipMemcpy D2H");
    hip_check(hipStreamSynchronize(nullptr), "saxs_debye");
    std::copy(result.begin(), result.end(), intensity);
}

void saxs_fit(size_t n, size_t n_q, const double *intensity, const double *i_exp, const double *sigma, double *scale_out, double *chi2_out) {
    if (n_q < 1 || n_q > (size_t)kSaxsMaxQ) throw Error(LD_ERR_INVALID, "n_q must be 1 .. 1024");
    if (!i_exp || !sigma) throw Error(LD_ERR_INVALID, "null argument");
    for (size_t j = 0; j < n_q; j++) {
        if (!std::isfinite(i_exp[j])) throw Error(LD_ERR_INVALID, "i_exp " + std::to_string(j) + " is not finite");
        if (!(sigma[j] > 0.0) || !std::isfinite(sigma[j])) throw Error(LD_ERR_INVALID, "sigma " + std::to_string(j) + " must be finite and > 0");
    }
    if (n == 0) return;
    if (!intensity) throw Error(LD_ERR_INVALID, "null argument");
    std::vector<double> scale(n), chi2(n);
    for (size_t i = 0; i < n; i++) {
        const double *I = intensity + i * n_q;
        double num = 0.0, den = 0.0;
        for (size_t j = 0; j < n_q; j++) {
            if (!std::isfinite(I[j])) throw Error(LD_ERR_INVALID, "intensity " + std::to_string(i) + ", " + std::to_string(j) + " is not finite");
            const double s2 = sigma[j] * sigma[j];
            num = num + i_exp[j] * I[j] / s2;
            den = den + I[j] * I[j] / s2;
        }
        if (den == 0.0 || !std::isfinite(den) || !std::isfinite(num)) throw Error(LD_ERR_INVALID, "pose " + std::to_string(i) + ": the scale's denominator is zero or not finite");
        scale[i] = num / den;
        double sum = 0.0;
        for (size_t j = 0; j < n_q; j++) {
            const double r = (i_exp[j] - scale[i] * I[j]) / sigma[j];
            sum = sum + r * r;
        }
        chi2[i] = sum / (double)n_q;
    }
    if (scale_out) std::copy(scale.begin(), scale.end(), scale_out);
    if (chi2_out) std::copy(chi2.begin(), chi2.end(), chi2_out);
}

// --- a complex ---------------------------------------------------------------------------------------------------------

void Complex::init_saxs() {
    std::vector<uint32_t> part_atom;
    std::vector<uint8_t> part_class;
    const PdbFile *files[2] = {&rec_, &lig_};
    for (int side = 0; side < 2; side++) {
        for (size_t a = 0; a < files[side]->lines.size(); a++) {
            const uint8_t e = saxs_class(files[side]->lines[a].data(), files[side]->lines[a].size());
            saxs_class_[side].push_back(e);
            if (e == kSaxsNoPart) continue;
            part_atom.push_back((uint32_t)(side * rec_.lines.size() + a));
            part_class.push_back(e);
            saxs_class_atoms_[e]++;
        }
        if (side == 0) saxs_.n_part_rec = (int)part_atom.size();
    }
    saxs_.n_part = (int)part_atom.size();
    saxs_.part_atom = arena_.upload(part_atom);
    saxs_.part_class = arena_.upload(part_class);
}

void Complex::saxs_classes(int side, uint8_t *class_out) const {
    side_file(side);
    if (!class_out) throw Error(LD_ERR_INVALID, "null argument");
    std::copy(saxs_class_[side].begin(), saxs_class_[side].end(), class_out);
}

void Complex::distance_histogram(size_t n, const double *poses, size_t stride, uint32_t width, size_t bins, uint32_t *counts) {
    saxs_run(n, poses, stride, width, bins, nullptr, 0, nullptr, counts);
}

void Complex::saxs(size_t n, const double *poses, size_t stride, uint32_t width, size_t bins, const double *q, size_t n_q,
                   double *intensity, uint32_t *counts) {
    check_q(q, n_q);
    saxs_run(n, poses, stride, width, bins, q, n_q, intensity, counts);
}

// The counts of n poses in chunks and, with q, the Debye sum over every chunk while it is on the device.  Nothing
// reaches the caller before the overflow flag is known.
void Complex::saxs_run(size_t n, const double *poses, size_t stride, uint32_t width, size_t bins, const double *q, size_t n_q,
                       double *intensity, uint32_t *counts) {
    check_grid(width, bins);
    const SaxsDevice &d = saxs_;
    if (d.n_part == 0) throw Error(LD_ERR_INVALID, "no atom of the complex takes part in the scattering (none of H, C, N, O, P, S outside MMB residues)");
    if (d.n_part > kSaxsMaxAtoms) throw Error(LD_ERR_INVALID, "more than 65536 atoms take part: a bin count would not fit 32 bits");
    if (n == 0) return;
    check_poses(n, poses, stride);
    const bool debye = q != nullptr;
    const size_t row_words = (size_t)kSaxsPairClasses * bins, row_bytes = row_words * sizeof(uint32_t);
    const size_t atom_bytes = (size_t)d.n_part * sizeof(int4);
    // without receptor modes the receptor's own pairs are the same for every pose: one base row a call
    const bool base = dev_.anm_rec == 0 && d.n_part_rec >= 2;
    const int first_b = base ? d.n_part_rec : 0;
    const size_t chunk = saxs_chunk_ ? std::min(saxs_chunk_, std::min<size_t>(n, 65535)) : chunk_of(row_bytes + atom_bytes, n, 65535);
    SaxsTables tables;
    if (debye) tables = saxs_tables(q, n_q, width, bins, saxs_class_atoms_);
    std::vector<uint32_t> h_counts(counts ? n * row_words : 0);

    upload_poses(n, poses, stride);
    int4 *d_atoms, *d_rec_atoms;  // the receptor's own atoms: null without `base`
    int *d_overflow;
    DeviceTables t;
    double *d_intensity;  // without q: n_q is 0 and the tables are empty, so these are null
    carve_into(d_ws_, [&](Carver &c) { d_atoms = c.take<int4>(chunk * (size_t)d.n_part), d_rec_atoms = c.take<int4>(base ? (size_t)d.n_part_rec : 0); });
    reserve_exact(d_out_, (chunk + 1) * row_bytes);  // one array: the rows of a chunk, then the base row
    uint32_t *d_counts = static_cast<uint32_t *>(d_out_.ptr), *d_base = d_counts + chunk * row_words;
    carve_into(d_ids_, [&](Carver &c) { d_overflow = c.take<int>(1), t = take_tables(tables, c), d_intensity = c.take<double>(n * n_q); });
    SaxsDebye sum;
    if (debye) {
        upload_tables(tables, t, stream_);
        sum.bins = (int)bins;
        sum.n_q = (int)n_q;
        sum.counts = d_counts;
        sum.sinc_t = t.sinc_t, sum.self = t.self, sum.cross = t.cross;
    }
    const double *d_poses = static_cast<const double *>(d_poses_.ptr);
    SaxsHistogram h;
    h.width = width;
    h.bins = (int)bins;
    h.overflow = d_overflow;
    begin_timed(d_overflow);
    if (base) {
        hip_check(launch_saxs_pose(dev_, d, d_poses, stride, 1, 0, d.n_part_rec, d_rec_atoms, (size_t)d.n_part_rec, d_overflow, stream_), "saxs_pose launch");
        hip_check(launch_saxs_rows(nullptr, d_base, 1, row_words, stream_), "saxs_rows launch");
        h.n_atoms = d.n_part_rec;
        h.first_b = 0;
        h.splits = saxs_splits(h.n_atoms, 0, 1);
        h.atoms = d_rec_atoms;
        h.atom_stride = (size_t)d.n_part_rec;
        h.counts = d_base;
        hip_check(launch_saxs_histogram(h, 1, stream_), "saxs_histogram launch");
    }
    h.n_atoms = d.n_part;
    h.first_b = first_b;
    h.atoms = d_atoms;
    h.atom_stride = (size_t)d.n_part;
    h.counts = d_counts;
    for (size_t i0 = 0; i0 < n; i0 += chunk) {
        const size_t m = std::min(chunk, n - i0);
        hip_check(launch_saxs_pose(dev_, d, d_poses + i0 * stride, stride, m, 0, d.n_part, d_atoms, (size_t)d.n_part, d_overflow, stream_), "saxs_pose launch");
        hip_check(launch_saxs_rows(base ? d_base : nullptr, d_counts, m, row_words, stream_), "saxs_rows launch");
        h.splits = saxs_splits(h.n_atoms, h.first_b, m);
        hip_check(launch_saxs_histogram(h, m, stream_), "saxs_histogram launch");
        if (debye) {
            sum.intensity = d_intensity + i0 * n_q;
            hip_check(launch_saxs_debye(sum, m, stream_), "saxs_debye launch");
        }
        if (counts) hip_check(hipMemcpyAsync(h_counts.data() + i0 * row_words, d_counts, m * row_bytes, hipMemcpyDeviceToHost, stream_), "hipMemcpy D2H counts");
    }
    finish_timed(d_overflow, "saxs", "a pair of atoms lies beyond the last bin, or a posed coordinate beyond +-1.0e6 A");
    if (intensity) hip_check(hipMemcpy(intensity, d_intensity, n * n_q * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy D2H");
    if (counts) std::copy(h_counts.begin(), h_counts.end(), counts);
}

}  // namespace ld
