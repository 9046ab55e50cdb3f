// nimpress_internal.hpp -- what the host's translation units share with each other and with nobody else
// (nimpress_text.cpp, the reader units over nimpress_readers.hpp, nimpress_scoring.cpp, nimpress_hooks.cpp).  The interface
// of the host is nimpress_host.hpp; the functions declared here are not exported from libnimpress_host.so.
#pragma once
#include "nimpress_host.hpp"

#include <charconv>
#include <cmath>
#include <cstring>

#pragma GCC visibility push(hidden)
namespace nimpress {

// ---- nimpress_text.cpp ----------------------------------------------------------------------------------
std::vector<std::string> splitChar(const std::string &s, char sep);
int64_t parseIntNim(const std::string &s);
bool readFile(const std::string &path, std::string &out);
double nowSeconds();

// ---- nimpress_scoring.cpp: one score row through getImputedDosages' early returns (nim:523-585) -----------
// What the reference decides about a row before it looks at a genotype, in its order: uncovered (nim:526-531), absent
// (:533-551), FILTER (:553-558), else the effect allele's index (:375-379).
struct RowClass {
    int kind = 0;                // 0 = genotyped, else NPS_ROW_UNCOVERED / _ABSENT / _FILTERED
    const Variant *v = nullptr;  // the record found (null for uncovered and absent rows)
    int ref_is_effect = 0;
    int eaidx = 0;               // genotyped rows: 0 = REF, k = ALT[k - 1]
    int code_map = 0;            // genotyped .bed / .pgen rows: the NPS_MAP_* that makes the 2-bit code an effect allele count
    std::string filter;          // FILTER of a filtered row's record (for the warning text)
    std::string pre_warning;     // emitted before the row's own warning (coverage contig, one FORMAT/DS value per sample)
};
RowClass classifyRow(const ScoreEntry &e, bool restrictToCoveredRgns, const GenomeIntervals &coveredIvals,
                     const RecordIndex &index, bool ignoreFilterField);
// the reference's warnings of one row (nim:527-579): the pre-warning, then at most one of the five texts.  neffect is
// the effect allele count as tallied (a float64 sum for FORMAT/DS rows: the test takes it rounded, the text prints
// neffect / nobs as it stands); over_maxmis is the caller's nim:565 decision.
void writeRowWarnings(Log &log, const ScoreEntry &e, int kind, const std::string &filter, const std::string &pre_warning,
                      int64_t nsamples, uint64_t nmissing, double neffect, bool over_maxmis, double afMismatchPthresh);

// getRawDosages (nim:367-391) on the host, for the one-pass route over FORMAT/DS files (computePolygenicScoresMulti with
// acceptDs), whose cohort holds float32 rows: a record scored from GT becomes the row of its effect allele's counts.
// gts: the typed FORMAT/GT vector as the record holds it (elem_bytes 1 / 2 / 4, n x ploidy values, (allele + 1) << 1 |
// phased).  Per sample: any missing allele gives NaN; vector-end pads (negative values) are skipped; else the number of
// alleles equal to eaidx, for any ploidy -- the rule of the device decoders (decode_gt_to_ds_kernel).
void decodeGtDosage(const void *gts, int elem_bytes, size_t n, int ploidy, int eaidx, float *out);
// the same for the 2-bit codes of a .bed / .pgen record under its code map (NPS_MAP_*)
void decodeCodeDosage(const uint8_t *codes, size_t n, int code_map, float *out);
// The host mirror of decode_pl_kernel (include/nps.h above nps_push_pl: same table -- nps_pl_likelihoods --, same order,
// same rules), for the one-pass dosage route and the CPU tests.  pl: the typed FORMAT/PL vector (elem_bytes 1 / 2 / 4) of n
// diploid samples, G = A (A + 1) / 2 values each for A = n_alleles (2 .. 8), genotype (j, k), j <= k, at k (k + 1) / 2 + j.
// Per sample: NaN when any value is negative (missing, end of vector) or the vector is flat; else with
// w_g = T[min(PL_g, 255)] the float32 of sum_g ((j == eaidx) + (k == eaidx)) w_g / sum_g w_g, both sums float64 in
// ascending g.
void decodePlDosage(const void *pl, int elem_bytes, size_t n, int n_alleles, int eaidx, float *out);

}  // namespace nimpress
#pragma GCC visibility pop

namespace nimpress {
// formatFloat into buf (at most 32 characters): their number.  Inline: the matrix writer formats millions of values.
inline size_t formatFloatTo(double x, char *buf) {
    if (std::isnan(x)) {
        memcpy(buf, "nan", 3);
        return 3;
    }
    if (std::isinf(x)) {
        const size_t n = x > 0 ? 3 : 4;
        memcpy(buf, x > 0 ? "inf" : "-inf", n);
        return n;
    }
    char *end = std::to_chars(buf, buf + 30, x, std::chars_format::general, 16).ptr;
    bool plain = true;
    for (const char *p = buf; p < end; ++p) plain = plain && *p != '.' && *p != 'e' && *p != 'n';
    if (plain) {
        *end++ = '.';
        *end++ = '0';
    }
    return (size_t)(end - buf);
}

// (default visibility: its inline destructor is among the library's weak symbols)
struct Tick {  // adds the scope's wall time to one of the Timings fields
    double &acc;
    double t0;
    explicit Tick(double &a) : acc(a), t0(nowSeconds()) {}
    ~Tick() { acc += nowSeconds() - t0; }
};
}  // namespace nimpress
