// nps_scale.h -- the fixed-point weight scales of a score definition: which rows the strip kernels cannot carry, the
// magnitude bands and the scale exponent of the others, and the one scale per score of a multi-score definition.
//
// Host only, pure functions of the row descriptors: no HIP, no device code, never included by a kernel source.  The units
// that build definitions (nps_resident.hip, nps_multiscore.hip) turn these plans into copies, uploads and error texts;
// tests/native/scale_driver.cpp compiles this header alone with plain g++ and tests/test_weight_scale.py holds it to
// tests/exact_reference.py (strip_scale, strip_bands, multi_scale) bit for bit.  The operand order and the types of every
// floating-point expression here decide bits of the scores.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/nps.h"

#pragma GCC visibility push(hidden)  // (inline functions of a shared library's units: nothing here is exported)
namespace nps {

constexpr int kMxBandBits = 30, kMxMaxBands = 8;

// the largest |imputed dosage - code| scale of a row: max(2, 2 |eaf|); a NaN eaf imputes NaN, which bounds nothing
inline double imputation_span(double eaf) { return std::isfinite(eaf) ? std::max(2.0, 2.0 * std::fabs(eaf)) : 2.0; }

// A PRESENT row the fixed-point kernels of NPS_FMT_GT2X cohorts cannot carry: a non-finite beta (0 x inf is NaN, every
// other dosage +-inf), an infinite eaf (the products of an imputed dosage are +-inf, and the kernels keep one NaN flag per
// row), or a weight bound |beta| (4 + max(2, 2 |eaf|)) outside [2^-900, 2^1000): beyond the fixed-point scale 2^F,
// |F| <= 1000, and beyond the overflow of the bound itself.  A NaN eaf is not special: its products are NaN.
inline bool mx_special(const nps_row_desc &r, double *bound) {
    *bound = 0.0;
    if (!std::isfinite(r.beta) || std::isinf(r.eaf)) return true;
    *bound = std::fabs(r.beta) * (4.0 + imputation_span(r.eaf));
    return r.beta != 0.0 && !(*bound >= 0x1p-900 && *bound < 0x1p1000);
}

// fixed-point scale 2^F of a strip pass: every weight of the band below 2^56 (fourteen hexadecimal digits)
inline int mx_scale_exponent(double bound) {
    if (!(bound > 0.0)) return 56;
    int e2 = 0;
    (void)std::frexp(bound, &e2);  // bound < 2^e2
    return std::min(1000, std::max(-1000, 56 - e2));
}

// The strip kernels' view of a definition's m PRESENT rows.  The special rows are scored at beta = eaf = 0 (band 0, part of
// no bound).  When the other weights span more than 2^30 (a sample that carries only its small-beta rows would see the
// quantisation of the largest one) they fall into magnitude bands of 2^30 below mx_bound: band b holds the rows with
// mx_bound 2^-30(b+1) < v <= mx_bound 2^-30b, the last band everything below.  A zero beta is in band 0.
struct MxBandPlan {
    std::vector<uint64_t> special;   // indices of the special rows, ascending
    double mx_bound = 0.0;           // the largest weight bound over the rows that are not special
    std::vector<int> band;           // [m] band of every row
    std::vector<int> used;           // the bands that cost a pass, ascending: band 0 always, the others when not empty
    std::vector<double> used_bound;  // ... and the largest weight bound of each (0: band 0 without a non-zero beta)
};

inline MxBandPlan mx_band_plan(const nps_row_desc *rows, uint64_t m) {
    MxBandPlan p;
    std::vector<int> band(m, 0);
    std::vector<double> v(m, 0.0);  // weight bound per row; 0 for a special row
    for (uint64_t j = 0; j < m; ++j) {
        double bound = 0.0;
        if (mx_special(rows[j], &bound)) {
            p.special.push_back(j);
            continue;
        }
        v[j] = bound;
        p.mx_bound = std::max(p.mx_bound, bound);
    }
    double band_bound[kMxMaxBands] = {0.0};
    bool any[kMxMaxBands] = {true};  // an empty band costs no pass, band 0 counts nloci and writes the statistics
    if (p.mx_bound > 0.0) {
        int e_top = 0;
        (void)std::frexp(p.mx_bound, &e_top);
        for (uint64_t j = 0; j < m; ++j) {
            if (v[j] == 0.0) continue;  // special, or beta = 0 (a non-zero beta that is not special has v >= 2^-900)
            int e_v = 0;
            (void)std::frexp(v[j], &e_v);
            const int b = band[j] = std::min(kMxMaxBands - 1, std::max(0, (e_top - e_v) / kMxBandBits));
            band_bound[b] = std::max(band_bound[b], v[j]);
            any[b] = true;
        }
    }
    for (int b = 0; b < kMxMaxBands; ++b)
        if (any[b]) {
            p.used.push_back(b);
            p.used_bound.push_back(band_bound[b]);
        }
    p.band.swap(band);
    return p;
}

// One fixed-point scale per score of a multi-score definition of S x n_desc rows with ND base-256 digits per weight: a
// weight is rounded to 2^-(8 ND - 9) of the largest one (x 5 for the imputation range), so a sample that carries only the
// score's SMALL-beta rows keeps 1e-6 relative only while 2.5 max|beta| / min|beta| <= 1e-6 x 2^(8 ND - 9): 2^25 for seven
// digits, 2^17 for six.  Beyond that the definition is refused -- the single-score path scores such a definition in
// magnitude bands -- instead of silently losing those samples.
struct MultiScale {
    enum Refusal { None = 0, BadKind, BetaNotFinite, EafInfinite, Span };
    Refusal refusal = None;  // the first refusal, in the order score, row; Span after the rows of its score
    int score = 0;           // ... its score
    uint64_t row = 0;        // ... and row (not Span)
    double minb = 0.0, maxb = 0.0;  // Span: the smallest non-zero and the largest |beta| of the score
    int F[NPS_MULTI_MAX_SCORES] = {0};  // weight * 2^F is an integer below 2^(8 ND - 9)
    int no_scale = -1;  // first score whose weight bound is not finite (|beta| = DBL_MAX): no fixed-point scale
};

inline int multi_span_bits(int ND) { return ND == 7 ? 25 : 17; }

inline MultiScale multi_scale(const nps_row_desc *rows, int n_scores, uint64_t n_desc, int ND) {
    MultiScale m;
    auto refuse = [&m](MultiScale::Refusal why, int s, uint64_t j) {
        m.refusal = why;
        m.score = s;
        m.row = j;
        return m;
    };
    for (int s = 0; s < n_scores; ++s) {
        double maxb = 0.0, maxe = 0.0, minb = HUGE_VAL;
        for (uint64_t j = 0; j < n_desc; ++j) {
            const nps_row_desc &r = rows[(uint64_t)s * n_desc + j];
            if (r.kind < NPS_ROW_PRESENT || r.kind > NPS_ROW_NOT_IN_SCORE) return refuse(MultiScale::BadKind, s, j);
            if (r.kind == NPS_ROW_NOT_IN_SCORE) continue;
            if (!std::isfinite(r.beta)) return refuse(MultiScale::BetaNotFinite, s, j);
            // (its imputed products are +-inf: the kernels keep one NaN flag; a NaN eaf is scored)
            if (std::isinf(r.eaf)) return refuse(MultiScale::EafInfinite, s, j);
            maxb = std::max(maxb, std::fabs(r.beta));
            if (r.beta != 0.0) minb = std::min(minb, std::fabs(r.beta));
            if (std::isfinite(r.eaf)) maxe = std::max(maxe, std::fabs(r.eaf));
        }
        const double span_limit = std::ldexp(1.0, multi_span_bits(ND));
        if (maxb > 0.0 && maxb / minb > span_limit) {
            m.minb = minb;
            m.maxb = maxb;
            return refuse(MultiScale::Span, s, 0);
        }
        // largest weight a row can have: |beta| * max(|imputed - 3|, |locus constant|)
        const double bound = maxb * (3.0 + std::max(2.0, 2.0 * maxe));
        // Finite betas whose bound overflows (|beta| = DBL_MAX) have no scale: frexp leaves e unspecified, and the weights
        // beta x 2^F would not be integers llrint can hold.  The dosage formats score such a definition in plain float64,
        // so it is not refused here but by nps_score_cohort_multi on a NPS_FMT_GT2M cohort.
        int e = 0;
        if (!std::isfinite(bound)) {
            if (m.no_scale < 0) m.no_scale = s;
        } else if (bound > 0.0) {
            (void)std::frexp(bound, &e);  // bound < 2^e
        }
        m.F[s] = 8 * ND - 9 - e;  // the kernel's coefficients (up to 160 x weight) stay below 2^(8 ND - 1)
    }
    return m;
}

}  // namespace nps
#pragma GCC visibility pop
