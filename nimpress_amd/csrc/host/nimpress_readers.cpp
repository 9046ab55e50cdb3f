// nimpress_readers.cpp -- see nimpress_host.hpp.  The host's genotype file readers: inflate, the text record parser,
// BGZF, tabix, BCF, CSI, the indexed sources with their parallel fetch, the PLINK filesets, and the record lookup
// (findVariant, RecordIndex).  No libnps symbol is referenced.
#include "nimpress_internal.hpp"

#include <zlib.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <thread>
#include <unordered_map>

namespace nimpress {

// ------------------------------------------------------------------------------------------
// VCF reader (text; plain or gzip/BGZF)
static bool inflateAll(const std::string &in, std::string &out) {
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, 15 + 32) != Z_OK) return false;  // gzip or zlib header, auto-detected
    zs.next_in = (Bytef *)in.data();
    zs.avail_in = (uInt)std::min<size_t>(in.size(), std::numeric_limits<uInt>::max());
    size_t consumed_total = 0;
    std::vector<char> buf(1 << 20);
    out.clear();
    while (true) {
        zs.next_out = (Bytef *)buf.data();
        zs.avail_out = (uInt)buf.size();
        const int rc = inflate(&zs, Z_NO_FLUSH);
        out.append(buf.data(), buf.size() - zs.avail_out);
        if (rc == Z_STREAM_END) {
            // BGZF = concatenated gzip members: continue with the next one if input remains
            consumed_total = in.size() - zs.avail_in;
            if (consumed_total >= in.size()) break;
            if (inflateReset(&zs) != Z_OK) {
                inflateEnd(&zs);
                return false;
            }
            continue;
        }
        if (rc != Z_OK) {
            inflateEnd(&zs);
            return false;
        }
        if (zs.avail_in == 0 && zs.avail_out != 0) break;  // truncated input: keep what we have
    }
    inflateEnd(&zs);
    return true;
}

static const int32_t kVectorEnd = (int32_t)0x80000001u;

// FORMAT/DS instead of FORMAT/GT for records that carry both: NIMPRESS_FORMAT=DS (a record without GT is scored
// from its DS in any case)
static bool preferDS() {
    const char *e = getenv("NIMPRESS_FORMAT");
    return e && (strcmp(e, "DS") == 0 || strcmp(e, "ds") == 0);
}
static float missingFloat() {  // the BCF2 missing float (0x7F800001): a NaN, which is what nps_push_ds calls missing
    const uint32_t u = 0x7F800001u;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static bool isVectorEndFloat(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u == 0x7F800002u;
}

const float *Variant::dsRow(int eaidx, size_t n, std::vector<float> &tmp) const {
    if (ds_per_sample == 1 && eaidx <= 1) return ds.data();
    tmp.assign(n, missingFloat());
    for (size_t i = 0; i < n; ++i) {
        const float *p = &ds[i * (size_t)ds_per_sample];
        if (eaidx >= 1) {
            if (eaidx <= ds_per_sample && !isVectorEndFloat(p[eaidx - 1])) tmp[i] = p[eaidx - 1];
        } else {  // effect allele = REF: 2 - (sum of the ALT dosages); a missing value makes the sample missing
            float sum = 0.0f;
            for (int k = 0; k < ds_per_sample; ++k)
                if (!isVectorEndFloat(p[k])) sum += p[k];
            if (sum > 2.0f) {  // the ALT dosages of a diploid sample add up to at most 2 (rounding of printed values aside)
                if (sum > 2.001f)
                    throw std::runtime_error("FORMAT/DS: the ALT dosages of a sample add up to more than 2 at " + contig + ":" +
                                             std::to_string(pos));
                sum = 2.0f;
            }
            tmp[i] = sum;
        }
    }
    return tmp.data();
}

// one sample's GT subfield -> alleles in the bcf_get_genotypes encoding
static int encodeGT(const char *p, const char *end, int32_t *out, int cap) {
    int n = 0;
    bool phased = false;
    const char *a = p;
    while (true) {
        const char *b = a;
        while (b < end && *b != '/' && *b != '|') ++b;
        int32_t v;
        if (b == a || (b - a == 1 && *a == '.')) {
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

// FORMAT/PL instead of GT / DS for records that carry it and have 2 .. 8 alleles: NIMPRESS_FORMAT=PL (opt-in only: with
// the variable unset or DS, PL is ignored)
static bool preferPL() {
    const char *e = getenv("NIMPRESS_FORMAT");
    return e && (strcmp(e, "PL") == 0 || strcmp(e, "pl") == 0);
}
static const int32_t kPlMissing = (int32_t)0x80000000u;

// The FORMAT/PL subfields (index pli) of the ns sample columns starting at s -> v.pl_raw as int32, G = A (A + 1) / 2 values
// per sample, parsed in place.  "." or an empty field makes the whole sample missing (a "." inside a list that one value);
// a short vector is padded with the end-of-vector value; a value beyond int32 is held as INT32_MAX (the decode caps at
// 255); a non-integer and a vector longer than G are errors naming the record.
static void parseTextPl(const char *s, const char *end, size_t ns, int pli, int n_alleles, Variant &v) {
    const int G = n_alleles * (n_alleles + 1) / 2;
    const std::string at = v.contig + ":" + std::to_string(v.pos);
    v.has_gt = false;
    v.has_ds = false;
    v.has_pl = true;
    v.pl_per_sample = G;
    v.pl_bytes = 4;
    std::vector<int32_t> vals(ns * (size_t)G);
    int32_t *dst = vals.data();
    for (size_t i = 0; i < ns; ++i, dst += G) {
        const char *t = s;
        while (t < end && *t != '\t') ++t;
        const char *g0 = s;  // pli-th ':' separated subfield of [s, t)
        for (int k = 0; k < pli && g0 < t; ++k) {
            while (g0 < t && *g0 != ':') ++g0;
            if (g0 < t) ++g0;
        }
        const char *g1 = g0;
        while (g1 < t && *g1 != ':') ++g1;
        for (int k = 0; k < G; ++k) dst[k] = kVectorEnd;
        if (g0 == g1 || (g1 - g0 == 1 && *g0 == '.')) {
            for (int k = 0; k < G; ++k) dst[k] = kPlMissing;
        } else {
            const char *a = g0;
            for (int k = 0;; ++k) {
                const char *b = a;
                while (b < g1 && *b != ',') ++b;
                if (k >= G)
                    throw std::runtime_error("FORMAT/PL with more than " + std::to_string(G) + " values (" +
                                             std::to_string(n_alleles) + " alleles) at " + at);
                if (b == a || (b - a == 1 && *a == '.')) {
                    dst[k] = kPlMissing;
                } else {
                    int64_t x = 0;
                    for (const char *c = a; c < b; ++c) {
                        if (*c < '0' || *c > '9')
                            throw std::runtime_error("bad FORMAT/PL value '" + std::string(a, (size_t)(b - a)) + "' at " + at);
                        if (x <= INT32_MAX) x = x * 10 + (*c - '0');
                    }
                    dst[k] = x > INT32_MAX ? INT32_MAX : (int32_t)x;
                }
                if (b >= g1) break;
                a = b + 1;
            }
        }
        if (t >= end && i + 1 < ns) throw std::runtime_error("VCF record with too few sample columns");
        s = t + 1;
    }
    v.pl_raw.resize(vals.size() * sizeof(int32_t));
    if (!vals.empty()) memcpy(v.pl_raw.data(), vals.data(), v.pl_raw.size());
}

// One VCF data line -> Variant.  `wanted` (optional): keep only records overlapping one of its
// regions; returns false when the record is filtered out.
typedef std::unordered_map<std::string, std::vector<std::pair<int64_t, int64_t>>> RegionMap;

static bool parseRecordLine(const char *L, size_t len, size_t ns, const RegionMap *wanted,
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
    if (wanted) {
        bool want = false;
        auto it = wanted->find(v.contig);
        if (it != wanted->end()) {
            const int64_t rend = v.pos + (int64_t)v.ref.size() - 1;
            for (const auto &w : it->second)
                if (v.pos <= w.second && rend >= w.first) {
                    want = true;
                    break;
                }
        }
        if (!want) return false;
    }
    const std::string alt = field(4);
    if (alt != ".") v.alt = splitChar(alt, ',');
    v.filter = field(6);
    if (ns) {
        if (nc < 10) throw std::runtime_error("VCF record without sample columns");
        const std::vector<std::string> fmt = splitChar(field(8), ':');
        int gi = -1, di = -1;
        for (size_t k = 0; k < fmt.size(); ++k) {
            if (fmt[k] == "GT") gi = (int)k;
            if (fmt[k] == "DS") di = (int)k;
        }
        int pli = -1;
        if (preferPL())
            for (size_t k = 0; k < fmt.size(); ++k)
                if (fmt[k] == "PL") pli = (int)k;
        if (pli >= 0) {  // NIMPRESS_FORMAT=PL: a record that carries PL and has 2 .. 8 alleles is scored from it
            const int n_alleles = 1 + (int)v.alt.size();
            if (n_alleles >= 2 && n_alleles <= 8) {
                parseTextPl(col[9], end, ns, pli, n_alleles, v);
                return true;
            }
            if (n_alleles > 8 && gi < 0 && di < 0)
                throw std::runtime_error("FORMAT/PL of a record with " + std::to_string(n_alleles) +
                                         " alleles (at most 8) and no FORMAT/GT or FORMAT/DS at " + v.contig + ":" + field(1));
        }
        if (gi < 0 && di < 0)
            throw std::runtime_error("VCF record without FORMAT/GT (or FORMAT/DS) at " + v.contig + ":" + field(1));
        if (di >= 0 && (gi < 0 || preferDS())) {  // FORMAT/DS: one float per ALT allele and sample, "." = missing
            v.has_gt = false;
            v.has_ds = true;
            // two sweeps over the sample columns, no allocation per genotype: the widest value list decides the
            // stride (Number=1 or Number=A), then every value is parsed where it lies
            const char *const s_first = col[9];
            auto subfield = [&](const char *s0, const char *&g0, const char *&g1) -> const char * {
                const char *t = s0;
                while (t < end && *t != '\t') ++t;
                g0 = s0;
                for (int k = 0; k < di && g0 < t; ++k) {
                    while (g0 < t && *g0 != ':') ++g0;
                    if (g0 < t) ++g0;
                }
                g1 = g0;
                while (g1 < t && *g1 != ':') ++g1;
                return t;
            };
            int width = 1;
            {
                const char *s = s_first;
                for (size_t i = 0; i < ns; ++i) {
                    const char *g0, *g1;
                    const char *t = subfield(s, g0, g1);
                    int k = 1;
                    for (const char *q = g0; q < g1; ++q) k += *q == ',';
                    width = std::max(width, k);
                    if (t >= end && i + 1 < ns) throw std::runtime_error("VCF record with too few sample columns");
                    s = t + 1;
                }
            }
            v.ds_per_sample = width;
            uint32_t eov_bits = 0x7F800002u;
            float eov;
            memcpy(&eov, &eov_bits, 4);
            v.ds.assign(ns * (size_t)width, eov);
            const char *s = s_first;
            for (size_t i = 0; i < ns; ++i) {
                const char *g0, *g1;
                const char *t = subfield(s, g0, g1);
                float *dst = &v.ds[i * (size_t)width];
                const char *a = g0;  // comma separated values of [g0, g1)
                for (int k = 0;; ++k) {
                    const char *b = a;
                    while (b < g1 && *b != ',') ++b;
                    if (b == a || (b - a == 1 && *a == '.')) {
                        dst[k] = missingFloat();
                    } else {
                        char buf[64];
                        const size_t len = (size_t)(b - a);
                        if (len >= sizeof buf) throw std::runtime_error("bad FORMAT/DS value (too long)");
                        memcpy(buf, a, len);
                        buf[len] = 0;
                        char *ep = nullptr;
                        const float f = strtof(buf, &ep);
                        if (!ep || *ep) throw std::runtime_error(std::string("bad FORMAT/DS value '") + buf + "'");
                        // (a dosage is 0 <= DS <= 2, but the streamed nps_push_ds rows this reader feeds take any finite
                        //  value, and nps_cohort_upload itself marks rows outside the range for the resident single-read
                        //  kernel: only what no kernel can score -- an infinity -- is refused here.  ADVICE round 4.)
                        if (f == f && !(std::fabs(f) <= 3.0e38f))
                            throw std::runtime_error(std::string("FORMAT/DS value ") + buf + " is not finite at " + v.contig +
                                                     ":" + field(1));
                        dst[k] = f;
                    }
                    if (b >= g1) break;
                    a = b + 1;
                }
                s = t + 1;
            }
            return true;
        }
        const int cap = 8;
        tmp.assign(ns * cap, kVectorEnd);
        int ploidy = 0;
        const char *s = col[9];
        for (size_t i = 0; i < ns; ++i) {
            const char *t = s;
            while (t < end && *t != '\t') ++t;
            const char *g0 = s;  // gi-th ':' separated subfield of [s,t)
            for (int k = 0; k < gi && g0 < t; ++k) {
                while (g0 < t && *g0 != ':') ++g0;
                if (g0 < t) ++g0;
            }
            const char *g1 = g0;
            while (g1 < t && *g1 != ':') ++g1;
            const int na = encodeGT(g0, g1, &tmp[i * cap], cap);
            if (na > cap) throw std::runtime_error("ploidy above 8 is not supported");
            ploidy = std::max(ploidy, na);
            if (t >= end && i + 1 < ns) throw std::runtime_error("VCF record with too few sample columns");
            s = t + 1;
        }
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
    return true;
}

// ---- BGZF random access + tabix (.tbi) index: what hts-nim's vcf.query() does through htslib ----
namespace {

struct BgzfFile {
    FILE *f = nullptr;
    // small cache of inflated blocks keyed by compressed offset
    std::unordered_map<uint64_t, std::pair<std::string, uint32_t>> cache;  // data, compressed size
    ~BgzfFile() {
        if (f) fclose(f);
    }
    bool open(const std::string &path) {
        f = fopen(path.c_str(), "rb");
        return f != nullptr;
    }
    // inflate the BGZF block starting at compressed offset `coff`; returns false at EOF / on error
    bool block(uint64_t coff, const std::string **data, uint32_t *csize) {
        auto it = cache.find(coff);
        if (it == cache.end()) {
            unsigned char hdr[18];
            if (fseeko(f, (off_t)coff, SEEK_SET) != 0 || fread(hdr, 1, 18, f) != 18) return false;
            if (hdr[0] != 0x1f || hdr[1] != 0x8b || !(hdr[3] & 4)) return false;
            const unsigned xlen = hdr[10] | (hdr[11] << 8);
            std::vector<unsigned char> extra(xlen);
            if (fseeko(f, (off_t)coff + 12, SEEK_SET) != 0 || fread(extra.data(), 1, xlen, f) != xlen)
                return false;
            int bsize = -1;
            for (unsigned i = 0; i + 4 <= xlen;) {
                const unsigned slen = extra[i + 2] | (extra[i + 3] << 8);
                if (extra[i] == 'B' && extra[i + 1] == 'C' && slen == 2)
                    bsize = (extra[i + 4] | (extra[i + 5] << 8)) + 1;
                i += 4 + slen;
            }
            if (bsize < 0) return false;  // a plain gzip file, not BGZF
            const unsigned cdata = (unsigned)bsize - xlen - 12 - 8;
            std::vector<unsigned char> comp(cdata + 8);
            if (fread(comp.data(), 1, cdata + 8, f) != cdata + 8) return false;
            const uint32_t isize = comp[cdata + 4] | (comp[cdata + 5] << 8) | (comp[cdata + 6] << 16) |
                                   ((uint32_t)comp[cdata + 7] << 24);
            std::string out(isize, '\0');
            z_stream zs;
            memset(&zs, 0, sizeof zs);
            if (inflateInit2(&zs, -15) != Z_OK) return false;
            zs.next_in = comp.data();
            zs.avail_in = cdata;
            zs.next_out = (Bytef *)out.data();
            zs.avail_out = isize;
            const int rc = inflate(&zs, Z_FINISH);
            inflateEnd(&zs);
            if (rc != Z_STREAM_END) return false;
            if (cache.size() > 64) cache.clear();
            it = cache.emplace(coff, std::make_pair(std::move(out), (uint32_t)bsize)).first;
        }
        *data = &it->second.first;
        *csize = it->second.second;
        return true;
    }
    // read n bytes starting at virtual offset *voff (advances it); false at EOF / on a short read
    bool readBytes(uint64_t *voff, void *dst, size_t n) {
        uint64_t coff = *voff >> 16;
        uint32_t uoff = (uint32_t)(*voff & 0xffff);
        char *out = (char *)dst;
        while (n) {
            const std::string *d;
            uint32_t csize;
            if (!block(coff, &d, &csize)) return false;
            if (uoff >= d->size()) {
                if (d->empty()) {  // EOF marker (or an empty block): only fine if more data follows
                    const std::string *d2;
                    uint32_t c2;
                    if (!block(coff + csize, &d2, &c2)) return false;
                }
                coff += csize;
                uoff = 0;
                continue;
            }
            const size_t take = std::min(n, d->size() - uoff);
            memcpy(out, d->data() + uoff, take);
            out += take;
            n -= take;
            uoff += (uint32_t)take;
            if (uoff >= d->size()) {
                coff += csize;
                uoff = 0;
            }
        }
        *voff = (coff << 16) | uoff;
        return true;
    }
    // read one text line starting at virtual offset *voff (advances it); false at EOF
    bool readLine(uint64_t *voff, std::string &line) {
        line.clear();
        uint64_t coff = *voff >> 16;
        uint32_t uoff = (uint32_t)(*voff & 0xffff);
        while (true) {
            const std::string *d;
            uint32_t csize;
            if (!block(coff, &d, &csize)) return !line.empty();
            if (d->empty() && line.empty()) {  // EOF marker block
                uint64_t next = coff + csize;
                const std::string *d2;
                uint32_t c2;
                if (!block(next, &d2, &c2)) return false;
                coff = next;
                uoff = 0;
                continue;
            }
            const char *b = d->data() + uoff, *e = d->data() + d->size();
            const char *nl = (const char *)memchr(b, '\n', (size_t)(e - b));
            if (nl) {
                line.append(b, nl - b);
                uoff = (uint32_t)(nl + 1 - d->data());
                if (uoff >= d->size()) {
                    coff += csize;
                    uoff = 0;
                }
                *voff = (coff << 16) | uoff;
                if (!line.empty() && line.back() == '\r') line.pop_back();
                return true;
            }
            line.append(b, e - b);
            coff += csize;
            uoff = 0;
        }
    }
};

struct TabixIndex {
    struct Ref {
        std::unordered_map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>> bins;
        std::vector<uint64_t> linear;
    };
    std::unordered_map<std::string, Ref> refs;

    bool load(const std::string &path) {
        std::string raw, t;
        if (!readFile(path, raw) || !inflateAll(raw, t)) return false;
        if (t.size() < 36 || memcmp(t.data(), "TBI\1", 4) != 0) return false;
        size_t o = 4;
        auto i32 = [&]() {
            int32_t v;
            if (o + 4 > t.size()) throw std::runtime_error("truncated .tbi");
            memcpy(&v, t.data() + o, 4);
            o += 4;
            return v;
        };
        auto u64 = [&]() {
            uint64_t v;
            if (o + 8 > t.size()) throw std::runtime_error("truncated .tbi");
            memcpy(&v, t.data() + o, 8);
            o += 8;
            return v;
        };
        const int32_t n_ref = i32();
        for (int k = 0; k < 6; ++k) (void)i32();  // format, col_seq, col_beg, col_end, meta, skip
        const int32_t l_nm = i32();
        std::vector<std::string> names;
        for (size_t a = o; a < o + (size_t)l_nm;) {
            const char *c = t.data() + a;
            names.emplace_back(c);
            a += names.back().size() + 1;
        }
        o += (size_t)l_nm;
        for (int32_t r = 0; r < n_ref; ++r) {
            Ref ref;
            const int32_t n_bin = i32();
            for (int32_t b = 0; b < n_bin; ++b) {
                const uint32_t bin = (uint32_t)i32();
                const int32_t n_chunk = i32();
                auto &v = ref.bins[bin];
                for (int32_t c = 0; c < n_chunk; ++c) {
                    const uint64_t beg = u64(), end = u64();
                    v.emplace_back(beg, end);
                }
            }
            const int32_t n_intv = i32();
            for (int32_t k = 0; k < n_intv; ++k) ref.linear.push_back(u64());
            if ((size_t)r < names.size()) refs[names[(size_t)r]] = std::move(ref);
        }
        return true;
    }

    // chunks (virtual offset ranges) that may hold records overlapping [beg0, end0) (0-based)
    std::vector<std::pair<uint64_t, uint64_t>> query(const std::string &contig, int64_t beg0,
                                                     int64_t end0) const {
        std::vector<std::pair<uint64_t, uint64_t>> out;
        auto it = refs.find(contig);
        if (it == refs.end()) return out;
        const Ref &ref = it->second;
        if (beg0 < 0) beg0 = 0;
        if (end0 <= beg0) end0 = beg0 + 1;
        const int64_t e = end0 - 1;
        uint64_t min_off = 0;
        if (!ref.linear.empty()) {
            const size_t w = (size_t)(beg0 >> 14);
            min_off = ref.linear[std::min(w, ref.linear.size() - 1)];
        }
        std::vector<uint32_t> bins = {0};
        for (uint32_t k = 1 + (uint32_t)(beg0 >> 26); k <= 1 + (uint32_t)(e >> 26); ++k) bins.push_back(k);
        for (uint32_t k = 9 + (uint32_t)(beg0 >> 23); k <= 9 + (uint32_t)(e >> 23); ++k) bins.push_back(k);
        for (uint32_t k = 73 + (uint32_t)(beg0 >> 20); k <= 73 + (uint32_t)(e >> 20); ++k) bins.push_back(k);
        for (uint32_t k = 585 + (uint32_t)(beg0 >> 17); k <= 585 + (uint32_t)(e >> 17); ++k) bins.push_back(k);
        for (uint32_t k = 4681 + (uint32_t)(beg0 >> 14); k <= 4681 + (uint32_t)(e >> 14); ++k) bins.push_back(k);
        for (uint32_t b : bins) {
            auto bi = ref.bins.find(b);
            if (bi == ref.bins.end()) continue;
            for (const auto &c : bi->second)
                if (c.second > min_off) out.emplace_back(std::max(c.first, min_off), c.second);
        }
        std::sort(out.begin(), out.end());
        return out;
    }
};


// ---- BCF2 (htslib's binary VCF): header dictionaries + record decoding ----------------------
// Layout restated from the VCF/BCF specification (hts-specs VCFv4.3 section 6; the reference reads
// BCF through htslib 1.10.2, Dockerfile:32).  Only what the path needs is decoded: CHROM, POS, ID,
// alleles, FILTER and the FORMAT/GT vector, which is kept in the file's own width.
struct BcfHeader {
    std::vector<std::string> contigs;  // BCF_DT_CTG
    std::vector<std::string> ids;      // BCF_DT_ID: FILTER/INFO/FORMAT ids, PASS = 0
    std::vector<std::string> samples;

    static bool attr(const std::string &line, const char *key, std::string &out) {
        // value of key= inside <...>, honouring quotes
        const size_t lt = line.find('<');
        if (lt == std::string::npos) return false;
        size_t i = lt + 1;
        const std::string k = std::string(key) + "=";
        while (i < line.size()) {
            const size_t eq = line.find('=', i);
            if (eq == std::string::npos) return false;
            const std::string name = line.substr(i, eq - i);
            size_t j = eq + 1;
            std::string val;
            if (j < line.size() && line[j] == '"') {
                ++j;
                while (j < line.size() && line[j] != '"') {
                    if (line[j] == '\\' && j + 1 < line.size()) ++j;
                    val += line[j++];
                }
                ++j;
            } else {
                while (j < line.size() && line[j] != ',' && line[j] != '>') val += line[j++];
            }
            if (name + "=" == k) {
                out = val;
                return true;
            }
            i = j + 1;  // past ',' or '>'
        }
        return false;
    }

    void parse(const std::string &text) {
        std::vector<std::pair<long, std::string>> ctg, idl;  // (IDX or -1, name) in header order
        std::unordered_map<std::string, size_t> seen;
        idl.emplace_back(-1, "PASS");  // htslib always registers PASS first
        seen["PASS"] = 0;
        size_t a = 0;
        while (a < text.size()) {
            size_t b = text.find('\n', a);
            if (b == std::string::npos) b = text.size();
            std::string line = text.substr(a, b - a);
            while (!line.empty() && (line.back() == '\r' || line.back() == '\0')) line.pop_back();
            a = b + 1;
            if (line.compare(0, 6, "#CHROM") == 0) {
                const std::vector<std::string> cols = splitChar(line, '\t');
                for (size_t k = 9; k < cols.size(); ++k) samples.push_back(cols[k]);
                continue;
            }
            const bool is_ctg = line.compare(0, 9, "##contig=") == 0;
            const bool is_id = line.compare(0, 9, "##FILTER=") == 0 || line.compare(0, 7, "##INFO=") == 0 ||
                               line.compare(0, 9, "##FORMAT=") == 0;
            if (!is_ctg && !is_id) continue;
            std::string id, idx;
            if (!attr(line, "ID", id)) continue;
            const long ix = attr(line, "IDX", idx) ? atol(idx.c_str()) : -1;
            if (is_ctg) {
                ctg.emplace_back(ix, id);
            } else {
                auto it = seen.find(id);
                if (it == seen.end()) {
                    seen[id] = idl.size();
                    idl.emplace_back(ix, id);
                } else if (ix >= 0) {
                    idl[it->second].first = ix;
                }
            }
        }
        auto place = [](const std::vector<std::pair<long, std::string>> &src, std::vector<std::string> &dst) {
            size_t next = 0;
            for (const auto &e : src) {
                const size_t at = e.first >= 0 ? (size_t)e.first : next;
                if (dst.size() <= at) dst.resize(at + 1);
                dst[at] = e.second;
                next = at + 1;
            }
        };
        place(ctg, contigs);
        place(idl, ids);
    }
};

struct BcfCursor {
    const unsigned char *p, *end;
    void need(size_t n) const {
        if ((size_t)(end - p) < n) throw std::runtime_error("truncated BCF record");
    }
    uint8_t u8() {
        need(1);
        return *p++;
    }
    int32_t intOf(int type) {  // one value of an integer type, sign extended
        switch (type) {
        case 1: {
            need(1);
            const int8_t v = (int8_t)*p;
            p += 1;
            return v;
        }
        case 2: {
            need(2);
            int16_t v;
            memcpy(&v, p, 2);
            p += 2;
            return v;
        }
        case 3: {
            need(4);
            int32_t v;
            memcpy(&v, p, 4);
            p += 4;
            return v;
        }
        default: throw std::runtime_error("BCF: integer expected");
        }
    }
    // typed-value descriptor: element type and count
    void desc(int &type, int64_t &len) {
        const uint8_t b = u8();
        type = b & 0xf;
        len = b >> 4;
        if (len == 15) {
            int t2;
            int64_t l2;
            desc(t2, l2);
            if (l2 != 1) throw std::runtime_error("BCF: bad length descriptor");
            len = intOf(t2);
            if (len < 0) throw std::runtime_error("BCF: negative length");
        }
    }
    static size_t sizeOf(int type) {
        switch (type) {
        case 0: return 0;
        case 1: case 7: return 1;
        case 2: return 2;
        case 3: case 5: return 4;
        default: throw std::runtime_error("BCF: unknown value type");
        }
    }
    std::string str() {
        int type;
        int64_t len;
        desc(type, len);
        if (type == 0) return std::string();
        if (type != 7) throw std::runtime_error("BCF: string expected");
        need((size_t)len);
        std::string s((const char *)p, (size_t)len);
        p += len;
        const size_t z = s.find('\0');
        if (z != std::string::npos) s.resize(z);
        return s;
    }
    int32_t typedInt() {
        int type;
        int64_t len;
        desc(type, len);
        if (len != 1) throw std::runtime_error("BCF: scalar integer expected");
        return intOf(type);
    }
};

// one record (shared + indiv blocks, without the two length words) -> Variant; returns false when
// `wanted` is given and the record overlaps none of its regions (nothing else is decoded then)
static bool parseBcfRecord(const unsigned char *shared, size_t l_shared, const unsigned char *indiv,
                           size_t l_indiv, const BcfHeader &h, const RegionMap *wanted, Variant &v) {
    BcfCursor c{shared, shared + l_shared};
    c.need(24);
    int32_t chrom, pos0, rlen;
    uint32_t nai, nfs;
    memcpy(&chrom, c.p, 4);
    memcpy(&pos0, c.p + 4, 4);
    memcpy(&rlen, c.p + 8, 4);
    memcpy(&nai, c.p + 16, 4);
    memcpy(&nfs, c.p + 20, 4);
    c.p += 24;
    const uint32_t n_allele = nai >> 16, n_fmt = nfs >> 24, n_sample = nfs & 0xffffff;
    if (chrom < 0 || (size_t)chrom >= h.contigs.size()) throw std::runtime_error("BCF: CHROM out of range");
    v = Variant();
    v.contig = h.contigs[(size_t)chrom];
    v.pos = (int64_t)pos0 + 1;
    if (wanted) {  // by the record's own span (POS .. POS + rlen - 1), before anything is copied
        bool want = false;
        auto it = wanted->find(v.contig);
        if (it != wanted->end()) {
            const int64_t rend = v.pos + std::max<int64_t>(rlen, 1) - 1;
            for (const auto &w : it->second)
                if (v.pos <= w.second && rend >= w.first) {
                    want = true;
                    break;
                }
        }
        if (!want) return false;
    }
    v.id = c.str();
    if (v.id.empty()) v.id = ".";
    for (uint32_t k = 0; k < n_allele; ++k) {
        std::string al = c.str();
        if (k == 0)
            v.ref = al;
        else
            v.alt.push_back(al);
    }
    {  // FILTER: vector of dictionary indices; empty = "."
        int type;
        int64_t len;
        c.desc(type, len);
        if (type == 0 || len == 0) {
            v.filter = ".";
        } else {
            for (int64_t k = 0; k < len; ++k) {
                const int32_t ix = c.intOf(type);
                if (ix < 0 || (size_t)ix >= h.ids.size()) throw std::runtime_error("BCF: FILTER id out of range");
                if (k) v.filter += ';';
                v.filter += h.ids[(size_t)ix];
            }
        }
    }
    // INFO is not needed; FORMAT fields
    v.has_gt = false;
    v.gts.clear();
    if (n_sample != h.samples.size()) throw std::runtime_error("BCF: record sample count differs from the header");
    BcfCursor f{indiv, indiv + l_indiv};
    int ds_type = 0;
    int64_t ds_len = 0;
    const unsigned char *ds_ptr = nullptr;
    size_t ds_bytes = 0;
    const unsigned char *gt_ptr = nullptr;
    size_t gt_nbytes = 0;
    const bool prefer_pl = preferPL();
    bool has_pl = false;
    int pl_type = 0;
    int64_t pl_len = 0;
    const unsigned char *pl_ptr = nullptr;
    size_t pl_bytes = 0;
    for (uint32_t k = 0; k < n_fmt; ++k) {
        const int32_t key = f.typedInt();
        int type;
        int64_t len;
        f.desc(type, len);
        const size_t bytes = BcfCursor::sizeOf(type) * (size_t)len * n_sample;
        f.need(bytes);
        if (key >= 0 && (size_t)key < h.ids.size() && h.ids[(size_t)key] == "GT") {
            if (type < 1 || type > 3) throw std::runtime_error("BCF: FORMAT/GT is not an integer vector");
            if (len > 8) throw std::runtime_error("ploidy above 8 is not supported");
            v.ploidy = (int)len;
            v.gt_bytes = type == 1 ? 1 : (type == 2 ? 2 : 4);
            gt_ptr = f.p;  // copied below, and only when the record is scored from its GT
            gt_nbytes = bytes;
            v.has_gt = true;
        } else if (key >= 0 && (size_t)key < h.ids.size() && h.ids[(size_t)key] == "DS") {
            // remembered only: whether the record is scored from GT or from DS is decided below, and a DS that is not
            // used is neither validated nor copied (a file with an oddly typed DS next to its GT scores as before)
            ds_type = type;
            ds_len = len;
            ds_ptr = f.p;
            ds_bytes = bytes;
            v.has_ds = true;
        } else if (prefer_pl && key >= 0 && (size_t)key < h.ids.size() && h.ids[(size_t)key] == "PL") {
            // remembered like DS: validated and copied only when the record is scored from it
            pl_type = type;
            pl_len = len;
            pl_ptr = f.p;
            pl_bytes = bytes;
            has_pl = true;
        }
        f.p += bytes;
    }
    if (has_pl && n_sample) {  // NIMPRESS_FORMAT=PL: a record that carries PL and has 2 .. 8 alleles is scored from it
        const int64_t n_alleles = 1 + (int64_t)v.alt.size();
        const std::string at = v.contig + ":" + std::to_string(v.pos);
        if (n_alleles >= 2 && n_alleles <= 8) {
            if (pl_type < 1 || pl_type > 3) throw std::runtime_error("BCF: FORMAT/PL is not an int8, int16 or int32 vector at " + at);
            if (pl_len != n_alleles * (n_alleles + 1) / 2)
                throw std::runtime_error("BCF: FORMAT/PL holds " + std::to_string(pl_len) + " values per sample, " +
                                         std::to_string(n_alleles * (n_alleles + 1) / 2) + " expected for " +
                                         std::to_string(n_alleles) + " alleles at " + at);
            v.has_pl = true;
            v.pl_per_sample = (int)pl_len;
            v.pl_bytes = pl_type == 1 ? 1 : (pl_type == 2 ? 2 : 4);
            v.pl_raw.assign(pl_ptr, pl_ptr + pl_bytes);
            v.has_gt = false;
            v.has_ds = false;
            return true;
        }
        if (n_alleles > 8 && !v.has_gt && !v.has_ds)
            throw std::runtime_error("FORMAT/PL of a record with " + std::to_string(n_alleles) +
                                     " alleles (at most 8) and no FORMAT/GT or FORMAT/DS at " + at);
    }
    if (n_sample && !v.has_gt && !v.has_ds)
        throw std::runtime_error("BCF record without FORMAT/GT (or FORMAT/DS) at " + v.contig + ":" + std::to_string(v.pos));
    if (v.has_ds && (!v.has_gt || preferDS())) {  // the selection rule of nimpress_host.hpp: one of the two is kept
        // typed float vector: len values per sample, missing 0x7F800001, end of vector 0x7F800002
        if (ds_type != 5) throw std::runtime_error("BCF: FORMAT/DS is not a float vector");
        if (ds_len < 1) throw std::runtime_error("BCF: empty FORMAT/DS vector");
        v.ds_per_sample = (int)ds_len;
        v.ds.resize((size_t)ds_len * n_sample);
        memcpy(v.ds.data(), ds_ptr, ds_bytes);
        for (const float x : v.ds)  // (NaN patterns = missing / end of vector; any finite value is scored: see the text reader)
            if (x == x && !(std::fabs(x) <= 3.0e38f))
                throw std::runtime_error("FORMAT/DS value " + std::to_string(x) + " is not finite at " + v.contig + ":" +
                                         std::to_string(v.pos));
        v.has_gt = false;
    } else {
        v.has_ds = false;
        if (v.has_gt) v.gt_raw.assign(gt_ptr, gt_ptr + gt_nbytes);
    }
    return true;
}

// CSI index (htslib's generalisation of tabix; what `bcftools index` writes for BCF)
struct CsiIndex {
    int32_t min_shift = 14, depth = 5;
    std::vector<std::unordered_map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>>> refs;

    bool load(const std::string &path) {
        std::string raw, t;
        if (!readFile(path, raw) || !inflateAll(raw, t)) return false;
        if (t.size() < 16 || memcmp(t.data(), "CSI\1", 4) != 0) return false;
        size_t o = 4;
        auto i32 = [&]() {
            int32_t v;
            if (o + 4 > t.size()) throw std::runtime_error("truncated .csi");
            memcpy(&v, t.data() + o, 4);
            o += 4;
            return v;
        };
        auto u64 = [&]() {
            uint64_t v;
            if (o + 8 > t.size()) throw std::runtime_error("truncated .csi");
            memcpy(&v, t.data() + o, 8);
            o += 8;
            return v;
        };
        min_shift = i32();
        depth = i32();
        const int32_t l_aux = i32();
        if (l_aux < 0 || o + (size_t)l_aux > t.size()) throw std::runtime_error("truncated .csi");
        o += (size_t)l_aux;
        const int32_t n_ref = i32();
        refs.resize((size_t)std::max(n_ref, 0));
        for (int32_t r = 0; r < n_ref; ++r) {
            const int32_t n_bin = i32();
            for (int32_t b = 0; b < n_bin; ++b) {
                const uint32_t bin = (uint32_t)i32();
                (void)u64();  // loffset
                const int32_t n_chunk = i32();
                auto &v = refs[(size_t)r][bin];
                for (int32_t k = 0; k < n_chunk; ++k) {
                    const uint64_t beg = u64(), end = u64();
                    v.emplace_back(beg, end);
                }
            }
        }
        return true;
    }

    std::vector<std::pair<uint64_t, uint64_t>> query(size_t ref, int64_t beg0, int64_t end0) const {
        std::vector<std::pair<uint64_t, uint64_t>> out;
        if (ref >= refs.size()) return out;
        if (beg0 < 0) beg0 = 0;
        if (end0 <= beg0) end0 = beg0 + 1;
        const int64_t e = end0 - 1;
        int s = min_shift + depth * 3;
        uint64_t t = 0;
        for (int l = 0; l <= depth; ++l) {
            const uint64_t b0 = t + (uint64_t)(beg0 >> s), b1 = t + (uint64_t)(e >> s);
            for (uint64_t b = b0; b <= b1; ++b) {
                auto bi = refs[ref].find((uint32_t)b);
                if (bi == refs[ref].end()) continue;
                for (const auto &c : bi->second) out.push_back(c);
            }
            t += 1ull << (l * 3);
            s -= 3;
        }
        std::sort(out.begin(), out.end());
        return out;
    }
};

static void bcfReadHeader(const unsigned char *p, size_t n, BcfHeader &h, size_t *body) {
    if (n < 9 || memcmp(p, "BCF\2", 4) != 0) throw std::runtime_error("not a BCF2 file");
    uint32_t l_text;
    memcpy(&l_text, p + 5, 4);
    if (9 + (size_t)l_text > n) throw std::runtime_error("truncated BCF header");
    h.parse(std::string((const char *)p + 9, l_text));
    *body = 9 + (size_t)l_text;
}

}  // namespace

// ---- indexed sources: vcf.gz + .tbi and BCF + .csi ------------------------------------------------
// What hts-nim's vcf.query() (nim:358) needs: the header and the index.  Records are fetched per set
// of score rows; every fetching thread inflates through a BGZF handle of its own.
struct IndexedSource {
    std::string path;
    bool is_bcf = false;
    BcfHeader bcf;
    std::unordered_map<std::string, size_t> bcf_contig;
    CsiIndex csi;
    TabixIndex tbi;
    size_t n_samples = 0;
};

namespace {

static unsigned hostThreads(size_t work_items) {
    unsigned t = std::thread::hardware_concurrency();
    if (t == 0) t = 4;
    t = std::min(t, 16u);
    if (const char *e = getenv("NIMPRESS_THREADS"))
        if (atoi(e) > 0) t = (unsigned)atoi(e);
    return (unsigned)std::max<size_t>(1, std::min<size_t>(t, work_items / 4 + 1));
}

// records overlapping entries [first, first+count), keyed by virtual offset (= file order)
static void fetchRange(const IndexedSource &src, const ScoreEntry *first, size_t count,
                       std::map<uint64_t, Variant> &found) {
    BgzfFile bg;
    if (!bg.open(src.path)) throw std::runtime_error("cannot open " + src.path);
    RegionMap wanted;
    for (size_t i = 0; i < count; ++i) wanted[first[i].contig].emplace_back(first[i].pos, first[i].stop());
    std::vector<unsigned char> buf;
    std::vector<int32_t> tmp;
    std::string line;
    // Where the scan of an index chunk stopped for the previous score row, so that a score file with many
    // loci in one 16 kb bin does not inflate and parse the bin from its start for every row: the scan of
    // chunk `beg` may resume at `at` if no record before `at` can overlap the new row, i.e. the row starts
    // beyond the end of every record passed so far (`max_end`, 1-based inclusive).
    struct Resume {
        uint64_t at;
        int64_t max_end;
    };
    std::unordered_map<uint64_t, Resume> resume;
    for (size_t i = 0; i < count; ++i) {
        const ScoreEntry &e = first[i];
        if (src.is_bcf) {
            auto ci = src.bcf_contig.find(e.contig);
            if (ci == src.bcf_contig.end()) continue;
            for (const auto &chunk : src.csi.query(ci->second, e.pos - 1, e.stop())) {
                uint64_t v = chunk.first;
                int64_t max_end = 0;
                auto rs = resume.find(chunk.first);
                if (rs != resume.end() && e.pos > rs->second.max_end) {
                    v = rs->second.at;
                    max_end = rs->second.max_end;
                }
                while (v < chunk.second) {
                    const uint64_t at = v;
                    uint32_t ls[2];
                    if (!bg.readBytes(&v, ls, 8)) break;
                    buf.resize((size_t)ls[0] + ls[1]);
                    if (!bg.readBytes(&v, buf.data(), buf.size())) throw std::runtime_error("truncated BCF record");
                    if (ls[0] < 24) continue;
                    int32_t chrom, pos0, rlen;
                    memcpy(&chrom, buf.data(), 4);
                    memcpy(&pos0, buf.data() + 4, 4);
                    memcpy(&rlen, buf.data() + 8, 4);
                    if ((size_t)chrom != ci->second) continue;
                    if ((int64_t)pos0 + 1 > e.stop()) {  // position sorted inside a contig
                        resume[chunk.first] = Resume{at, max_end};
                        break;
                    }
                    max_end = std::max(max_end, (int64_t)pos0 + std::max(rlen, 1));
                    if (found.count(at)) continue;
                    Variant var;
                    if (parseBcfRecord(buf.data(), ls[0], buf.data() + ls[0], ls[1], src.bcf, &wanted, var))
                        found.emplace(at, std::move(var));
                }
            }
        } else {
            for (const auto &chunk : src.tbi.query(e.contig, e.pos - 1, e.stop())) {
                uint64_t v = chunk.first;
                int64_t max_end = 0;
                auto rs = resume.find(chunk.first);
                if (rs != resume.end() && e.pos > rs->second.max_end) {
                    v = rs->second.at;
                    max_end = rs->second.max_end;
                }
                while (v < chunk.second) {
                    const uint64_t at = v;
                    if (!bg.readLine(&v, line)) break;
                    if (line.empty() || line[0] == '#') continue;
                    // cheap pre-check of CHROM and POS before the full parse
                    const size_t t1 = line.find('\t');
                    const size_t t2 = t1 == std::string::npos ? t1 : line.find('\t', t1 + 1);
                    if (t2 == std::string::npos) continue;
                    if (line.compare(0, t1, e.contig) != 0) continue;
                    const int64_t pos = parseIntNim(line.substr(t1 + 1, t2 - t1 - 1));
                    if (pos > e.stop()) {  // records are position sorted inside a contig
                        resume[chunk.first] = Resume{at, max_end};
                        break;
                    }
                    {  // end of the record: POS + len(REF) - 1 (REF is the fourth column)
                        const size_t t3 = line.find('\t', t2 + 1);
                        const size_t t4 = t3 == std::string::npos ? t3 : line.find('\t', t3 + 1);
                        const int64_t reflen = t4 == std::string::npos ? 1 : (int64_t)(t4 - t3 - 1);
                        max_end = std::max(max_end, pos + std::max<int64_t>(reflen, 1) - 1);
                    }
                    if (found.count(at)) continue;
                    Variant var;
                    if (parseRecordLine(line.data(), line.size(), src.n_samples, &wanted, tmp, var))
                        found.emplace(at, std::move(var));
                }
            }
        }
    }
}

static std::vector<Variant> fetchParallel(const IndexedSource &src, const ScoreEntry *first, size_t count) {
    Tick tick(timings().inflate_parse);
    const unsigned nt = hostThreads(count);
    std::vector<std::map<uint64_t, Variant>> parts(nt);
    if (nt <= 1) {
        fetchRange(src, first, count, parts[0]);
    } else {
        std::vector<std::thread> th;
        std::vector<std::exception_ptr> err(nt);
        const size_t per = (count + nt - 1) / nt;
        for (unsigned t = 0; t < nt; ++t) {
            const size_t a = std::min(count, (size_t)t * per), b = std::min(count, a + per);
            th.emplace_back([&, t, a, b]() {
                try {
                    if (b > a) fetchRange(src, first + a, b - a, parts[t]);
                } catch (...) {
                    err[t] = std::current_exception();
                }
            });
        }
        for (auto &x : th) x.join();
        for (auto &e : err)
            if (e) std::rethrow_exception(e);
    }
    std::map<uint64_t, Variant> &all = parts[0];
    for (unsigned t = 1; t < nt; ++t)
        for (auto &kv : parts[t]) all.emplace(kv.first, std::move(kv.second));  // duplicates: first wins
    std::vector<Variant> out;
    out.reserve(all.size());
    for (auto &kv : all) out.push_back(std::move(kv.second));
    return out;
}

// header + index of an indexed file, or null
static std::shared_ptr<IndexedSource> openIndexed(const std::string &path, std::vector<std::string> &samples) {
    if (getenv("NIMPRESS_NO_INDEX")) return nullptr;
    auto src = std::make_shared<IndexedSource>();
    src->path = path;
    {  // BCF + CSI
        BgzfFile bg;
        if (bg.open(path)) {
            uint64_t voff = 0;
            unsigned char magic[9];
            if (bg.readBytes(&voff, magic, 9) && memcmp(magic, "BCF\2", 4) == 0 && src->csi.load(path + ".csi")) {
                uint32_t l_text;
                memcpy(&l_text, magic + 5, 4);
                std::string text(l_text, '\0');
                if (!bg.readBytes(&voff, &text[0], l_text)) throw std::runtime_error("truncated BCF header");
                src->bcf.parse(text);
                src->is_bcf = true;
                samples = src->bcf.samples;
                for (size_t k = 0; k < src->bcf.contigs.size(); ++k) src->bcf_contig[src->bcf.contigs[k]] = k;
                src->n_samples = samples.size();
                return src;
            }
        }
    }
    {  // vcf.gz + tabix
        BgzfFile bg;
        if (src->tbi.load(path + ".tbi") && bg.open(path)) {
            uint64_t voff = 0;
            std::string line;
            while (bg.readLine(&voff, line)) {  // header lines
                if (line.empty()) continue;
                if (line[0] != '#') break;
                if (line.compare(0, 6, "#CHROM") == 0) {
                    const std::vector<std::string> cols = splitChar(line, '\t');
                    samples.clear();
                    for (size_t k = 9; k < cols.size(); ++k) samples.push_back(cols[k]);
                    src->n_samples = samples.size();
                    return src;
                }
            }
        }
    }
    return nullptr;
}

}  // namespace

bool VCF::openStreaming(const std::string &path) {
    samples.clear();
    records.clear();
    source = openIndexed(path, samples);
    indexed = streaming = source != nullptr;
    return streaming;
}

std::vector<Variant> VCF::fetch(const ScoreEntry *first, size_t count) const {
    if (!source) throw std::runtime_error("VCF::fetch needs an indexed file");
    return fetchParallel(*source, first, count);
}

// ---- VCF::open in parts: the PLINK fileset reader, the whole-file BCF scan, the text scan (the indexed path is
// openIndexed + fetchParallel above).  `wanted` (optional): keep only records overlapping one of its regions.
// PLINK 1 fileset: <prefix>.bed + .bim + .fam, or PLINK 2: .pgen + .pvar + .psam.  False when `path` is neither.
static bool openPlinkFileset(const std::string &path, const RegionMap *wanted, std::vector<std::string> &samples,
                             std::vector<Variant> &records) {
    FILE *f = fopen(path.c_str(), "rb");
    unsigned char magic[3] = {0, 0, 0};
    const bool is_bed = f && fread(magic, 1, 3, f) == 3 && magic[0] == 0x6c && magic[1] == 0x1b;
    if (!is_bed) {
        if (f) fclose(f);
        return false;
    }
    struct Closer {
        FILE *f;
        ~Closer() { fclose(f); }
    } closer{f};
    // byte 3 = storage mode: 0x01 PLINK 1 .bed (variant-major), 0x02 PLINK 2 .pgen with fixed-width hard-call
    // records (12-byte header: magic, mode, uint32 variants, uint32 samples, one flag byte; then
    // ceil(N/4) bytes per variant, the 2-bit code = number of ALT alleles, 3 = missing).  Nothing else of
    // the .pgen family is read (variable-width records, dosages, multi-allelic hard calls).
    // PARITY UNPINNED: neither plink2 nor the format's specification is in this image; the layout is written
    // from the published description and pinned only by the build's own writer (tests/pgenwriter.py).
    const bool pgen = magic[2] == 2;
    if (magic[2] == 0) throw std::runtime_error("sample-major .bed files are not supported");
    if (magic[2] != 1 && !pgen)
        throw std::runtime_error("PLINK 2 .pgen storage mode 0x" + std::string(1, "0123456789abcdef"[magic[2] >> 4]) +
                                 std::string(1, "0123456789abcdef"[magic[2] & 15]) +
                                 " is not supported (only 0x02: fixed-width hard calls; plink2 --make-pgen fixed-width, "
                                 "or convert with --make-bed)");
    std::string prefix = path;
    if (prefix.size() > 4 && (prefix.compare(prefix.size() - 4, 4, ".bed") == 0)) prefix.resize(prefix.size() - 4);
    if (prefix.size() > 5 && (prefix.compare(prefix.size() - 5, 5, ".pgen") == 0)) prefix.resize(prefix.size() - 5);
    std::string fam, bim;
    bool pvar = false, psam = false;
    if (pgen) {  // .pvar / .psam, or the PLINK 1 .bim / .fam next to the .pgen
        pvar = readFile(prefix + ".pvar", bim);
        psam = readFile(prefix + ".psam", fam);
        if ((!pvar && !readFile(prefix + ".bim", bim)) || (!psam && !readFile(prefix + ".fam", fam)))
            throw std::runtime_error("cannot open " + prefix + ".pvar / .psam (or .bim / .fam) next to the .pgen file");
    } else if (!readFile(prefix + ".fam", fam) || !readFile(prefix + ".bim", bim)) {
        throw std::runtime_error("cannot open " + prefix + ".fam / .bim next to the .bed file");
    }
    size_t header_bytes = 3;
    uint32_t pgen_m = 0, pgen_n = 0;
    if (pgen) {
        unsigned char h[9];
        if (fread(h, 1, 9, f) != 9) throw std::runtime_error("truncated .pgen header");
        memcpy(&pgen_m, h, 4);
        memcpy(&pgen_n, h + 4, 4);
        header_bytes = 12;
    }
    auto fields = [](const std::string &line) {
        std::vector<std::string> out;
        size_t i = 0;
        while (i < line.size()) {
            while (i < line.size() && (line[i] == ' ' || line[i] == '\t' || line[i] == '\r')) ++i;
            size_t j = i;
            while (j < line.size() && line[j] != ' ' && line[j] != '\t' && line[j] != '\r') ++j;
            if (j > i) out.push_back(line.substr(i, j - i));
            i = j;
        }
        return out;
    };
    size_t iid_col = 1;  // .fam: FID IID ...; .psam: the column its header line calls IID
    for (const std::string &ln : splitChar(fam, '\n')) {
        const std::vector<std::string> c = fields(ln);
        if (c.empty()) continue;
        if (psam && c[0][0] == '#') {
            if (c[0] == "#IID") iid_col = 0;
            else if (c[0] == "#FID") iid_col = 1;
            else continue;  // other comment lines
            if (iid_col >= c.size() || (iid_col == 1 && c[1] != "IID")) throw std::runtime_error("bad .psam header line");
            continue;
        }
        if (c.size() <= iid_col) throw std::runtime_error(psam ? "bad .psam line" : "bad .fam line");
        samples.push_back(c[iid_col]);  // IID
    }
    if (pgen && pgen_n != samples.size())
        throw std::runtime_error(".pgen header says " + std::to_string(pgen_n) + " samples, the sample file lists " +
                                 std::to_string(samples.size()));
    const size_t row_bytes = (samples.size() + 3) / 4;
    size_t row = 0;
    // .pvar: '##' meta lines, then '#CHROM POS ID REF ALT ...' naming the columns; without that line the file
    // has the .bim layout (chrom, id, cM, pos, ALT = A1, REF = A2)
    int col_chrom = 0, col_id = 1, col_pos = 3, col_alt = 4, col_ref = 5;
    size_t min_cols = 6;
    for (const std::string &ln : splitChar(bim, '\n')) {
        const std::vector<std::string> c = fields(ln);
        if (c.empty()) continue;
        if (pvar && c[0].size() >= 2 && c[0][0] == '#' && c[0][1] == '#') continue;
        if (pvar && c[0][0] == '#' && c[0] != "#CHROM") continue;  // (any other comment line: not a record)
        if (pvar && c[0] == "#CHROM") {
            col_chrom = 0;
            col_id = col_pos = col_alt = col_ref = -1;
            for (size_t k = 1; k < c.size(); ++k) {
                if (c[k] == "POS") col_pos = (int)k;
                if (c[k] == "ID") col_id = (int)k;
                if (c[k] == "REF") col_ref = (int)k;
                if (c[k] == "ALT") col_alt = (int)k;
            }
            if (col_pos < 0 || col_ref < 0 || col_alt < 0) throw std::runtime_error(".pvar header line lacks POS / REF / ALT");
            min_cols = (size_t)std::max(std::max(col_pos, col_ref), std::max(col_alt, col_id)) + 1;
            continue;
        }
        if (c.size() < min_cols) throw std::runtime_error(pgen ? "bad .pvar / .bim line" : "bad .bim line");
        Variant v;
        v.contig = c[(size_t)col_chrom];
        v.id = col_id >= 0 ? c[(size_t)col_id] : ".";
        v.pos = parseIntNim(c[(size_t)col_pos]);
        v.ref = c[(size_t)col_ref];           // .bed: A2; .pgen: REF
        v.alt.push_back(c[(size_t)col_alt]);  // .bed: A1; .pgen: ALT
        if (pgen && v.alt[0].find(',') != std::string::npos)
            throw std::runtime_error("multi-allelic .pvar record at " + v.contig + ":" + std::to_string(v.pos) +
                                     ": not representable in fixed-width hard-call records");
        v.filter = ".";
        v.is_bed = !pgen;
        v.is_pgen = pgen;
        v.gt_bytes = 0;
        v.ploidy = 2;
        bool want = !wanted;
        if (wanted) {
            auto it = wanted->find(v.contig);
            if (it != wanted->end()) {
                const int64_t len = (int64_t)std::max(v.ref.size(), v.alt[0].size());
                for (const auto &w : it->second)
                    if (v.pos <= w.second && v.pos + len - 1 >= w.first) {
                        want = true;
                        break;
                    }
            }
        }
        if (want) {
            v.gt_raw.resize(row_bytes);
            if (row_bytes &&
                (fseeko(f, (off_t)(header_bytes + row * row_bytes), SEEK_SET) != 0 ||
                 fread(v.gt_raw.data(), 1, row_bytes, f) != row_bytes))
                throw std::runtime_error(pgen ? "truncated .pgen file" : "truncated .bed file");
            records.push_back(std::move(v));
        }
        ++row;
    }
    if (pgen) {
        // the records are mapped to rows by line index alone: a .pvar that does not belong to this .pgen would be
        // scored with another variant's genotypes, silently.  The header's variant count and the file's length
        // must both agree with what was read.
        if (row != pgen_m)
            throw std::runtime_error(".pgen header says " + std::to_string(pgen_m) + " variants, " + prefix +
                                     (pvar ? ".pvar" : ".bim") + " lists " + std::to_string(row));
        if (fseeko(f, 0, SEEK_END) != 0) throw std::runtime_error("cannot seek in the .pgen file");
        const off_t size = ftello(f);
        if ((uint64_t)size != (uint64_t)header_bytes + (uint64_t)pgen_m * row_bytes)
            throw std::runtime_error(".pgen file is " + std::to_string((long long)size) + " bytes, " +
                                     std::to_string(pgen_m) + " fixed-width records of " + std::to_string(samples.size()) +
                                     " samples are " + std::to_string((unsigned long long)header_bytes + (unsigned long long)pgen_m * row_bytes));
    }
    return true;
}

static void scanBcf(const std::string &text, const RegionMap *wanted, std::vector<std::string> &samples,
                    std::vector<Variant> &records) {
    BcfHeader h;
    size_t o = 0;
    const unsigned char *base = (const unsigned char *)text.data();
    bcfReadHeader(base, text.size(), h, &o);
    samples = h.samples;
    while (o + 8 <= text.size()) {
        uint32_t ls[2];
        memcpy(ls, base + o, 8);
        o += 8;
        if (o + (size_t)ls[0] + ls[1] > text.size()) throw std::runtime_error("truncated BCF record");
        Variant v;
        if (parseBcfRecord(base + o, ls[0], base + o + ls[0], ls[1], h, wanted, v))
            records.push_back(std::move(v));
        o += (size_t)ls[0] + ls[1];
    }
}

// false without a #CHROM header line
static bool scanText(const std::string &text, const RegionMap *wanted, std::vector<std::string> &samples,
                     std::vector<Variant> &records) {
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
                    std::vector<std::string> cols = splitChar(std::string(L, len), '\t');
                    for (size_t k = 9; k < cols.size(); ++k) samples.push_back(cols[k]);
                    have_header = true;
                }
            } else {
                if (!have_header) throw std::runtime_error("VCF record before the #CHROM header line");
                Variant v;
                if (parseRecordLine(L, len, samples.size(), wanted, tmp, v))
                    records.push_back(std::move(v));
            }
        }
        a = b + 1;
    }
    return have_header;
}

// open(): text VCF, plain or gzip/BGZF.  With `keep` and a tabix index next to a BGZF file
// (path + ".tbi") only the index chunks overlapping the score loci are inflated -- the random
// access hts-nim's vcf.query() performs (nim:358); otherwise the whole file is scanned.
bool VCF::open(const std::string &path, const std::vector<ScoreEntry> *keep) {
    samples.clear();
    records.clear();
    indexed = streaming = false;
    source.reset();
    RegionMap wanted;
    if (keep)
        for (const ScoreEntry &e : *keep) wanted[e.contig].emplace_back(e.pos, e.stop());
    const RegionMap *only = keep ? &wanted : nullptr;
    if (openPlinkFileset(path, only, samples, records)) return true;
    if (keep) {  // vcf.gz + .tbi / BCF + .csi: only the chunks of the wanted loci are inflated
        source = openIndexed(path, samples);
        if (source) {
            records = fetchParallel(*source, keep->data(), keep->size());
            indexed = true;
            return true;
        }
        samples.clear();
    }

    std::string raw;
    if (!readFile(path, raw)) return false;
    std::string text;
    if (raw.size() >= 2 && (unsigned char)raw[0] == 0x1f && (unsigned char)raw[1] == 0x8b) {
        if (!inflateAll(raw, text)) return false;
        raw.clear();
        raw.shrink_to_fit();
    } else {
        text.swap(raw);
    }
    if (text.size() >= 5 && text.compare(0, 3, "BCF") == 0) {  // whole-file scan of a BCF
        scanBcf(text, only, samples, records);
        return true;
    }
    return scanText(text, only, samples, records);
}

// element i as bcf_get_genotypes hands it out: int8 / int16 end-of-vector and missing become their
// int32 counterparts, everything else is sign extended (htslib vcf.c, bcf_get_format_values)
int32_t Variant::gtValue(size_t i) const {
    if (is_bed) {  // (diploid; A2 = allele 0, A1 = allele 1)
        const unsigned code = (gt_raw[(i / 2) >> 2] >> (((i / 2) & 3) * 2)) & 3u;
        if (code == 1) return 0;                       // missing
        const int n_a1 = code == 0 ? 2 : (code == 2 ? 1 : 0);
        return ((int)(i & 1) < n_a1 ? 2 : 1) << 1;     // (allele + 1) << 1
    }
    if (is_pgen) {  // (diploid; the code is the number of ALT alleles, 3 = missing)
        const unsigned code = (gt_raw[(i / 2) >> 2] >> (((i / 2) & 3) * 2)) & 3u;
        if (code == 3) return 0;
        return ((unsigned)(i & 1) < code ? 2 : 1) << 1;
    }
    if (gt_raw.empty()) return gts[i];
    switch (gt_bytes) {
    case 1: {
        const int8_t x = (int8_t)gt_raw[i];
        return x == (int8_t)0x81 ? (int32_t)0x80000001u : x == (int8_t)0x80 ? (int32_t)0x80000000u : x;
    }
    case 2: {
        int16_t x;
        memcpy(&x, &gt_raw[2 * i], 2);
        return x == (int16_t)0x8001 ? (int32_t)0x80000001u : x == (int16_t)0x8000 ? (int32_t)0x80000000u : x;
    }
    default: {
        int32_t x;
        memcpy(&x, &gt_raw[4 * i], 4);
        return x;
    }
    }
}

// nim:359-363 for one record that overlaps the query
static bool variantMatches(const Variant &v, const std::string &refseq, const std::string &easeq) {
    if (v.is_bed) {  // no REF in a .bim: the row's two alleles must be the variant's two alleles
        const std::string &a1 = v.alt[0], &a2 = v.ref;
        return (refseq == a2 && (easeq == a1 || easeq == a2)) || (refseq == a1 && (easeq == a1 || easeq == a2));
    }
    if (v.ref != refseq) return false;  // nim:359 -- POS itself is never compared
    if (easeq == refseq) return true;
    for (const std::string &a : v.alt)
        if (a == easeq) return true;
    return false;
}
static int64_t variantLen(const Variant &v) {
    return (int64_t)(v.is_bed ? std::max(v.ref.size(), v.alt[0].size()) : v.ref.size());
}

const Variant *findVariant(const std::string &contig, int64_t pos, const std::string &refseq,
                           const std::string &easeq, const VCF &vcf) {
    const int64_t stop = pos + (int64_t)refseq.size() - 1;
    for (const Variant &v : vcf.records) {  // file order = the order a region query returns
        if (v.contig != contig) continue;
        const int64_t vend = v.pos + variantLen(v) - 1;
        if (v.pos > stop || vend < pos) continue;
        if (variantMatches(v, refseq, easeq)) return &v;
    }
    return nullptr;
}

void RecordIndex::build(const std::vector<Variant> &recs) {
    contigs.clear();
    records = &recs;
    for (size_t i = 0; i < recs.size(); ++i) {
        Contig &c = contigs[recs[i].contig];
        if (!c.ids.empty() && recs[c.ids.back()].pos > recs[i].pos) c.sorted = false;
        c.ids.push_back((uint32_t)i);
        c.maxlen = std::max(c.maxlen, variantLen(recs[i]));
    }
}

const Variant *RecordIndex::find(const std::string &contig, int64_t pos, const std::string &refseq,
                                 const std::string &easeq) const {
    auto ci = contigs.find(contig);
    if (ci == contigs.end()) return nullptr;
    const Contig &c = ci->second;
    const std::vector<Variant> &recs = *records;
    const int64_t stop = pos + (int64_t)refseq.size() - 1;
    size_t a = 0, b = c.ids.size();
    if (c.sorted) {  // candidates start at pos - maxlen + 1 .. stop; the first match in file order wins
        const int64_t lo = pos - c.maxlen + 1;
        a = (size_t)(std::lower_bound(c.ids.begin(), c.ids.end(), lo,
                                      [&](uint32_t id, int64_t x) { return recs[id].pos < x; }) - c.ids.begin());
        b = (size_t)(std::upper_bound(c.ids.begin(), c.ids.end(), stop,
                                      [&](int64_t x, uint32_t id) { return x < recs[id].pos; }) - c.ids.begin());
    }
    for (size_t k = a; k < b; ++k) {
        const Variant &v = recs[c.ids[k]];
        const int64_t vend = v.pos + variantLen(v) - 1;
        if (v.pos > stop || vend < pos) continue;
        if (variantMatches(v, refseq, easeq)) return &v;
    }
    return nullptr;
}

}  // namespace nimpress
