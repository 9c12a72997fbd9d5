// saxs.hpp -- the host side of the SAXS profiles (lightdock_hip.h, "Small-angle scattering"): the tables
// the host makes with libm (form factors, sinc, the Debye sum's coefficients), the Debye sum on the caller's counts, and
// the fit.  What the header says of ld_saxs_* holds for the functions of the same names; refusals are ld::Error.  The
// methods of Complex that use them (saxs_classes, distance_histogram, saxs) are defined in saxs.cpp too.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace ld {

void saxs_form_factors(const double *q, size_t n_q, double *f_out);                              // n_q x 6
void saxs_sinc(const double *q, size_t n_q, uint32_t width, size_t bins, double *s_out);          // n_q x bins
void saxs_debye_host(size_t n, const uint32_t *counts, uint32_t width, size_t bins, const uint32_t *class_atoms, const double *q,
                     size_t n_q, double *intensity);
void saxs_fit(size_t n, size_t n_q, const double *intensity, const double *i_exp, const double *sigma, double *scale_out,
              double *chi2_out);

// What the Debye kernel reads, made on the host: s transposed (bins x n_q), S_j (n_q), F_{j,c} (n_q x 21).
struct SaxsTables {
    std::vector<double> sinc_t, self, cross;
};
SaxsTables saxs_tables(const double *q, size_t n_q, uint32_t width, size_t bins, const uint32_t *class_atoms);

}  // namespace ld
