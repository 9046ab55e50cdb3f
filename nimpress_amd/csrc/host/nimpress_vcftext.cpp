// nimpress_vcftext.cpp -- see nimpress_readers.hpp.  The text VCF record parser (FORMAT/GT, /DS and /PL, parsed where
// they lie), the whole-file text scan, and what the text and the BCF reader decide alike: which FORMAT field a record is
// scored from, and the sample names of a #CHROM line.
#include "nimpress_readers.hpp"

#include <algorithm>
#include <cstdlib>

namespace nimpress {

Format preferredFormat() {
    const char *e = getenv("NIMPRESS_FORMAT");
    if (e && (strcmp(e, "DS") == 0 || strcmp(e, "ds") == 0)) return Format::DS;
    if (e && (strcmp(e, "PL") == 0 || strcmp(e, "pl") == 0)) return Format::PL;
    return Format::GT;
}

Format scoredFrom(Format prefer, bool has_gt, bool has_ds, bool has_pl, int64_t n_alleles, const char *kind,
                  const std::string &at) {
    if (has_pl) {  // NIMPRESS_FORMAT=PL: a record that carries PL and has 2 .. 8 alleles is scored from it
        if (n_alleles >= 2 && n_alleles <= 8) return Format::PL;
        if (n_alleles > 8 && !has_gt && !has_ds)
            throw std::runtime_error("FORMAT/PL of a record with " + std::to_string(n_alleles) +
                                     " alleles (at most 8) and no FORMAT/GT or FORMAT/DS at " + at);
    }
    if (!has_gt && !has_ds)
        throw std::runtime_error(std::string(kind) + " record without FORMAT/GT (or FORMAT/DS) at " + at);
    return gtOrDs(prefer, has_gt, has_ds);
}

void sampleNames(const std::string &chrom_line, std::vector<std::string> &samples) {
    const std::vector<std::string> cols = splitChar(chrom_line, '\t');
    for (size_t k = 9; k < cols.size(); ++k) samples.push_back(cols[k]);
}

namespace {

const int32_t kVectorEnd = (int32_t)0x80000001u;
const int32_t kPlMissing = (int32_t)0x80000000u;

inline bool isMissingToken(const char *a, const char *b) { return b == a || (b - a == 1 && *a == '.'); }

// The ns sample columns (tab separated) from s to end: f(i, g0, g1) with [g0, g1) the k-th ':' separated sub-field of
// sample i (empty when the column has fewer).  Inline with its callable: this is the per-genotype loop of the text path.
// The three parsers that use it stay out of line (noinline): inlined into parseRecordLine together their loops spill.
template <class F>
__attribute__((always_inline)) inline void forEachSampleField(const char *s, const char *end, size_t ns, int k, F &&f) {
    for (size_t i = 0; i < ns; ++i) {
        const char *t = s;
        while (t < end && *t != '\t') ++t;
        const char *g0 = s;
        for (int j = 0; j < k && g0 < t; ++j) {
            while (g0 < t && *g0 != ':') ++g0;
            if (g0 < t) ++g0;
        }
        const char *g1 = g0;
        while (g1 < t && *g1 != ':') ++g1;
        f(i, g0, g1);
        if (t >= end && i + 1 < ns) throw std::runtime_error("VCF record with too few sample columns");
        s = t + 1;
    }
}

// The ',' separated values of [g0, g1): f(k, a, b, missing) for value k = [a, b), missing when it is empty or "."
template <class F> __attribute__((always_inline)) inline void forEachListValue(const char *g0, const char *g1, F &&f) {
    const char *a = g0;
    for (int k = 0;; ++k) {
        const char *b = a;
        while (b < g1 && *b != ',') ++b;
        f(k, a, b, isMissingToken(a, b));
        if (b >= g1) break;
        a = b + 1;
    }
}

// one sample's GT subfield -> alleles in the bcf_get_genotypes encoding
int encodeGT(const char *p, const char *end, int32_t *out, int cap) {
    int n = 0;
    bool phased = false;
    const char *a = p;
    while (true) {
        const char *b = a;
        while (b < end && !(*b == '/' || *b == '|')) ++b;
        int32_t v;
        if (isMissingToken(a, b)) {
            v = 0;  // missing allele
        } else {
            long k = 0;
            for (const char *c = a; c < b; ++c) {
                if (*c < '0' || *c > '9') throw std::runtime_error("bad GT allele");
                k = k * 10 + (*c - '0');
            }
            v = (int32_t)((k + 1) << 1);
        }
        if (phased) v |= 1;
        if (n < cap) out[n] = v;
        ++n;
        if (b >= end) break;
        phased = *b == '|';
        a = b + 1;
    }
    return n;
}

// FORMAT/GT (index gi) -> v.gt_raw / v.gts; `tmp` is the caller's scratch
__attribute__((noinline))
void parseTextGt(const char *s, const char *end, size_t ns, int gi, std::vector<int32_t> &tmp, Variant &v) {
    const int cap = 8;
    tmp.assign(ns * cap, kVectorEnd);
    int ploidy = 0;
    int32_t *const codes = tmp.data();
    forEachSampleField(s, end, ns, gi, [codes, &ploidy](size_t i, const char *g0, const char *g1) {
        const int na = encodeGT(g0, g1, codes + i * cap, cap);
        if (na > cap) throw std::runtime_error("ploidy above 8 is not supported");
        ploidy = std::max(ploidy, na);
    });
    v.ploidy = ploidy;
    // Kept the way a BCF record would hold it: int8 when every allele index fits (always, in
    // practice), so that a row costs `ploidy` bytes per sample in host memory and over PCIe.
    bool small = true;
    for (size_t i = 0; i < ns && small; ++i)
        for (int k = 0; k < ploidy; ++k) {
            const int32_t x = tmp[i * cap + k];
            if (x != kVectorEnd && x > 127) small = false;
        }
    if (small) {
        v.gt_bytes = 1;
        v.gt_raw.resize(ns * ploidy);
        for (size_t i = 0; i < ns; ++i)
            for (int k = 0; k < ploidy; ++k) {
                const int32_t x = tmp[i * cap + k];
                v.gt_raw[i * ploidy + k] = x == kVectorEnd ? (uint8_t)0x81 : (uint8_t)x;
            }
    } else {
        v.gts.resize(ns * ploidy);
        for (size_t i = 0; i < ns; ++i)
            for (int k = 0; k < ploidy; ++k) v.gts[i * ploidy + k] = tmp[i * cap + k];
    }
}

// The FORMAT/PL subfields (index pli) of the ns sample columns starting at s -> v.pl_raw as int32, G = A (A + 1) / 2 values
// per sample, parsed in place.  "." or an empty field makes the whole sample missing (a "." inside a list that one value);
// a short vector is padded with the end-of-vector value; a value beyond int32 is held as INT32_MAX (the decode caps at
// 255); a non-integer and a vector longer than G are errors naming the record.
__attribute__((noinline))
void parseTextPl(const char *s, const char *end, size_t ns, int pli, int n_alleles, Variant &v) {
    const int G = n_alleles * (n_alleles + 1) / 2;
    const std::string at = v.contig + ":" + std::to_string(v.pos);
    v.has_gt = false;
    v.has_ds = false;
    v.has_pl = true;
    v.pl_per_sample = G;
    v.pl_bytes = 4;
    std::vector<int32_t> vals(ns * (size_t)G);
    forEachSampleField(s, end, ns, pli, [&](size_t i, const char *g0, const char *g1) {
        int32_t *dst = &vals[i * (size_t)G];
        std::fill(dst, dst + G, isMissingToken(g0, g1) ? kPlMissing : kVectorEnd);
        if (isMissingToken(g0, g1)) return;
        forEachListValue(g0, g1, [&](int k, const char *a, const char *b, bool missing) {
            if (k >= G)
                throw std::runtime_error("FORMAT/PL with more than " + std::to_string(G) + " values (" +
                                         std::to_string(n_alleles) + " alleles) at " + at);
            if (missing) {
                dst[k] = kPlMissing;
                return;
            }
            int64_t x = 0;
            for (const char *c = a; c < b; ++c) {
                if (*c < '0' || *c > '9')
                    throw std::runtime_error("bad FORMAT/PL value '" + std::string(a, (size_t)(b - a)) + "' at " + at);
                if (x <= INT32_MAX) x = x * 10 + (*c - '0');
            }
            dst[k] = x > INT32_MAX ? INT32_MAX : (int32_t)x;
        });
    });
    v.pl_raw.resize(vals.size() * sizeof(int32_t));
    if (!vals.empty()) memcpy(v.pl_raw.data(), vals.data(), v.pl_raw.size());
}

// FORMAT/DS (index di): one float per ALT allele and sample, "." = missing.  Two sweeps over the sample columns, no
// allocation per genotype: the widest value list decides the stride (Number=1 or Number=A), then every value is parsed
// where it lies; a shorter list is padded with the end-of-vector value.
__attribute__((noinline))
void parseTextDs(const char *s, const char *end, size_t ns, int di, const std::string &at, Variant &v) {
    v.has_gt = false;
    v.has_ds = true;
    int width = 1;
    forEachSampleField(s, end, ns, di, [&](size_t, const char *g0, const char *g1) {
        width = std::max(width, 1 + (int)std::count(g0, g1, ','));
    });
    v.ds_per_sample = width;
    v.ds.assign(ns * (size_t)width, kDsEnd);
    forEachSampleField(s, end, ns, di, [&](size_t i, const char *g0, const char *g1) {
        float *dst = &v.ds[i * (size_t)width];
        forEachListValue(g0, g1, [&](int k, const char *a, const char *b, bool missing) {
            if (missing) {
                dst[k] = kDsMissing;
                return;
            }
            char buf[64];
            const size_t len = (size_t)(b - a);
            if (len >= sizeof buf) throw std::runtime_error("bad FORMAT/DS value (too long)");
            memcpy(buf, a, len);
            buf[len] = 0;
            char *ep = nullptr;
            const float f = strtof(buf, &ep);
            if (!ep || *ep) throw std::runtime_error(std::string("bad FORMAT/DS value '") + buf + "'");
            // (a dosage is 0 <= DS <= 2, but the streamed nps_push_ds rows this reader feeds take any finite value, and
            //  nps_cohort_upload itself marks rows outside the range for the resident single-read kernel: only what no
            //  kernel can score -- an infinity -- is refused here.  ADVICE round 4.)
            if (isInfiniteDs(f)) throw std::runtime_error(std::string("FORMAT/DS value ") + buf + " is not finite at " + at);
            dst[k] = f;
        });
    });
}

}  // namespace

bool parseRecordLine(const char *L, size_t len, size_t ns, const RegionMap *wanted, Format prefer,
                     std::vector<int32_t> &tmp, Variant &v) {
    const char *col[10];
    const char *p = L, *end = L + len;
    int nc = 0;
    col[nc++] = p;
    while (nc < 10 && p < end) {
        if (*p == '\t') col[nc++] = p + 1;
        ++p;
    }
    if (nc < 8) throw std::runtime_error("VCF record with fewer than 8 columns");
    auto field = [&](int k) {
        const char *s = col[k];
        const char *t = (k + 1 < nc) ? col[k + 1] - 1 : end;
        return std::string(s, t - s);
    };
    v = Variant();
    v.contig = field(0);
    v.pos = parseIntNim(field(1));
    v.id = field(2);
    v.ref = field(3);
    if (wanted && !overlapsWanted(*wanted, v.contig, v.pos, v.pos + (int64_t)v.ref.size() - 1)) return false;
    const std::string alt = field(4);
    if (alt != ".") v.alt = splitChar(alt, ',');
    v.filter = field(6);
    if (!ns) return true;
    if (nc < 10) throw std::runtime_error("VCF record without sample columns");
    const std::vector<std::string> fmt = splitChar(field(8), ':');
    int gi = -1, di = -1, pli = -1;
    for (size_t k = 0; k < fmt.size(); ++k) {
        if (fmt[k] == "GT") gi = (int)k;
        if (fmt[k] == "DS") di = (int)k;
        if (fmt[k] == "PL" && prefer == Format::PL) pli = (int)k;
    }
    const int n_alleles = 1 + (int)v.alt.size();
    const std::string at = v.contig + ":" + field(1);  // POS as the file writes it
    switch (scoredFrom(prefer, gi >= 0, di >= 0, pli >= 0, n_alleles, "VCF", at)) {
    case Format::PL: parseTextPl(col[9], end, ns, pli, n_alleles, v); break;
    case Format::DS: parseTextDs(col[9], end, ns, di, at, v); break;
    case Format::GT: parseTextGt(col[9], end, ns, gi, tmp, v); break;
    }
    return true;
}

bool scanText(const std::string &text, const RegionMap *wanted, std::vector<std::string> &samples,
              std::vector<Variant> &records) {
    const Format prefer = preferredFormat();
    std::vector<int32_t> tmp;
    bool have_header = false;
    size_t a = 0;
    const size_t n = text.size();
    while (a < n) {
        size_t b = text.find('\n', a);
        if (b == std::string::npos) b = n;
        size_t e = b;
        if (e > a && text[e - 1] == '\r') --e;  // CRLF (tests/set1.vcf.gz)
        if (e > a) {
            const char *L = text.data() + a;
            const size_t len = e - a;
            if (L[0] == '#') {
                if (len > 6 && memcmp(L, "#CHROM", 6) == 0) {
                    sampleNames(std::string(L, len), samples);
                    have_header = true;
                }
            } else {
                if (!have_header) throw std::runtime_error("VCF record before the #CHROM header line");
                Variant v;
                if (parseRecordLine(L, len, samples.size(), wanted, prefer, tmp, v))
                    records.push_back(std::move(v));
            }
        }
        a = b + 1;
    }
    return have_header;
}

}  // namespace nimpress
