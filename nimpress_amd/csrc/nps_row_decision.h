// nps_row_decision.h -- the decisions every score row goes through before any arithmetic (getImputedDosages,
// nimpress.nim:484-585), written once: plain C++ that is also device code (tests/native/decision_driver.cpp compiles it
// with g++; the kernels and the host's no-data rows call it -- all but ds_fused_kernel).  Internal header.
//
//   nmissing / nsamples > --maxmis   (:565)  a locus constant (imputeLocusDosages :417-447) for every sample, or
//                                            the row's own dosages with an imputed value for its missing samples
//   ngenotyped >= --mincs            (:471)  that value is the cohort's own frequency, or the fall-back
//
// Every expression keeps the reference's operand order, types and casts; the library is built with -ffp-contract=off,
// so host and device give the same bits.
#pragma once
#include <stdint.h>

#include "../../include/nps.h"

#ifdef __HIPCC__
#define NPS_ROW_FN __host__ __device__ __forceinline__
#else
#define NPS_ROW_FN inline
#endif

namespace nps {

struct DevParams {
    int32_t imp_locus, imp_missing, imp_sample;
    double max_missing_rate;
    double min_cs;  // compared in double, nimpress.nim:471
};

// the one NaN of an imputed dosage: the quiet NaN 0x7ff8000000000000, on host and device
NPS_ROW_FN double row_nan() { return __builtin_nan(""); }

// the reference's test `nmissing / N > --maxmis` (double division, nimpress.nim:565) is monotone in nmissing: the largest
// count that is NOT over the rate (-1: none), found with that very expression -- the kernels compare integers
NPS_ROW_FN int64_t maxmis_threshold(uint64_t n, double rate) {
    if (n == 0 || (double)0 / (double)n > rate) return -1;
    uint64_t lo = 0, hi = n;  // pred(lo) holds
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (!((double)mid / (double)n > rate))
            lo = mid;
        else
            hi = mid - 1;
    }
    return (int64_t)lo;
}

// nimpress.nim:565 itself, == nmissing > maxmis_threshold(n, rate) (tests/test_row_decision.py): the kernels whose
// control wave has no time for a float64 division compare with the threshold, the others divide
NPS_ROW_FN bool over_maxmis(uint64_t nmissing, uint64_t n, double rate) {
    const double missingrate = (double)nmissing / (double)n;
    return missingrate > rate;
}

// imputeLocusDosages nimpress.nim:417-447: the dosage of every sample of a row without usable genotypes; 0: row dropped
NPS_ROW_FN int locus_dosage(const DevParams &p, double eaf, bool rie, double &dosage) {
    dosage = 0.0;
    if (p.imp_locus == NPS_LOCUS_IGNORE) return 0;
    dosage = p.imp_locus == NPS_LOCUS_PS       ? eaf * 2.0
             : p.imp_locus == NPS_LOCUS_HOMREF ? (rie ? 2.0 : 0.0)
                                               : row_nan();
    return 1;
}

// imputeSampleDosages nimpress.nim:450-481: the dosage of a missing sample of a genotyped row.  neff: the effect
// alleles of the ngen genotyped samples (an exact count on the 2-bit paths, a dosage sum on the DS paths)
NPS_ROW_FN double sample_dosage(const DevParams &p, double eaf, bool rie, double neff, uint64_t ngen) {
    switch (p.imp_sample) {
    case NPS_SAMPLE_PS: return eaf * 2.0;
    case NPS_SAMPLE_HOMREF: return rie ? 2.0 : 0.0;
    case NPS_SAMPLE_FAIL: return row_nan();
    default:
        if ((double)ngen >= p.min_cs) return neff / (double)ngen;
        return p.imp_sample == NPS_SAMPLE_INT_PS ? eaf * 2.0 : row_nan();
    }
}

struct RowDecision {
    int used, reason;  // return value of getImputedDosages; nps_reason
    int mode;          // 0 dropped, 1 genotyped (imp = dosage of a missing sample), 2 locus constant (imp = every sample's dosage)
    double imp;
};

// a row with genotype data; over: nimpress.nim:565 as the caller spells it (over_maxmis, or nmissing > maxmis_threshold)
NPS_ROW_FN RowDecision decide_row(const DevParams &p, bool over, double eaf, bool rie, double neff, uint64_t ngen) {
    RowDecision d;
    if (over) {  // :565-571
        d.reason = NPS_REASON_MAXMIS;
        d.used = locus_dosage(p, eaf, rie, d.imp);
        d.mode = d.used ? 2 : 0;
    } else {  // :582-585
        d.reason = NPS_REASON_GENOTYPED;
        d.used = 1;
        d.mode = 1;
        d.imp = sample_dosage(p, eaf, rie, neff, ngen);
    }
    return d;
}

// a row without genotype data: NPS_ROW_ABSENT (:536-551, --imputemissing), UNCOVERED (:526-531) / FILTERED (:553-558)
NPS_ROW_FN RowDecision no_data_row(const DevParams &p, int kind, double eaf, bool rie) {
    RowDecision d;
    if (kind == NPS_ROW_ABSENT) {
        d.reason = NPS_REASON_ABSENT;
        d.used = p.imp_missing == NPS_MISSING_HOMREF ? 1 : 0;
        d.imp = d.used ? (rie ? 2.0 : 0.0) : 0.0;
    } else {
        d.reason = kind == NPS_ROW_UNCOVERED ? NPS_REASON_UNCOVERED : NPS_REASON_FILTERED;
        d.used = locus_dosage(p, eaf, rie, d.imp);
    }
    d.mode = d.used ? 2 : 0;
    return d;
}

NPS_ROW_FN nps_locus_stat row_stat(const RowDecision &d, uint64_t ngen, uint64_t nmiss, double neff) {
    nps_locus_stat s;
    s.ngenotyped = ngen;
    s.nmissing = nmiss;
    s.neffect = neff;
    s.used = d.used;
    s.reason = d.reason;
    return s;
}

}  // namespace nps
