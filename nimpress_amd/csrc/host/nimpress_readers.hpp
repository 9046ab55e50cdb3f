// nimpress_readers.hpp -- what the genotype file reader units share with each other and with nobody else:
// nimpress_bgzf.cpp (inflate, BGZF, the bin index), nimpress_vcftext.cpp (text records, the format rule),
// nimpress_bcf.cpp, nimpress_plink.cpp and nimpress_readers.cpp (the indexed sources, VCF::open / fetch, the record
// lookup).  None of them references a libnps symbol; nothing declared here is exported from libnimpress_host.so.
#pragma once
#include "nimpress_internal.hpp"

#include <cstdio>
#include <stdexcept>
#include <unordered_map>

#pragma GCC visibility push(hidden)
namespace nimpress {

// ---- regions: keep only records overlapping one of the score rows' spans (1-based, inclusive) -------------------------
typedef std::unordered_map<std::string, std::vector<std::pair<int64_t, int64_t>>> RegionMap;
// Does the record [first, last] on `contig` overlap a wanted region?  Each reader has its own rule for `last`: the text
// reader POS + len(REF) - 1, the BCF reader POS + max(rlen, 1) - 1, the PLINK reader POS + (the longer allele) - 1.
inline bool overlapsWanted(const RegionMap &wanted, const std::string &contig, int64_t first, int64_t last) {
    const auto it = wanted.find(contig);
    if (it == wanted.end()) return false;
    for (const auto &w : it->second)
        if (first <= w.second && last >= w.first) return true;
    return false;
}

// ---- the two float patterns of a FORMAT/DS vector (BCF2): both NaNs, which is what nps_push_ds calls missing ----------
inline float floatOfBits(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
inline const float kDsMissing = floatOfBits(0x7F800001u), kDsEnd = floatOfBits(0x7F800002u);
inline bool isDsEnd(float f) { return memcmp(&f, &kDsEnd, 4) == 0; }
// only what no kernel can score -- an infinity -- is refused by the readers (a NaN pattern is missing / end of vector)
inline bool isInfiniteDs(float f) { return f == f && !(std::fabs(f) <= 3.0e38f); }

// ---- nimpress_vcftext.cpp ---------------------------------------------------------------------------------------------
// Which FORMAT field records are scored from.  NIMPRESS_FORMAT=DS: FORMAT/DS instead of FORMAT/GT for records that carry
// both (a record without GT is scored from its DS in any case); =PL: FORMAT/PL instead of GT / DS for records that carry
// it and have 2 .. 8 alleles (opt-in only: otherwise PL is not even looked for).  Read once per scan or fetch.
enum class Format { GT, DS, PL };
Format preferredFormat();
inline Format gtOrDs(Format prefer, bool has_gt, bool has_ds) {
    return has_ds && (!has_gt || prefer == Format::DS) ? Format::DS : Format::GT;
}
// The rule for one record with samples: has_pl is asked only under Format::PL; kind is "VCF" or "BCF" and `at` the
// record's contig:pos, for the two refusals.
Format scoredFrom(Format prefer, bool has_gt, bool has_ds, bool has_pl, int64_t n_alleles, const char *kind,
                  const std::string &at);
// the sample names of a #CHROM header line, appended
void sampleNames(const std::string &chrom_line, std::vector<std::string> &samples);
// One VCF data line -> Variant; false when `wanted` is given and the record overlaps none of its regions.
bool parseRecordLine(const char *L, size_t len, size_t ns, const RegionMap *wanted, Format prefer,
                     std::vector<int32_t> &tmp, Variant &v);
// whole-file scan of a text VCF; false without a #CHROM header line
bool scanText(const std::string &text, const RegionMap *wanted, std::vector<std::string> &samples,
              std::vector<Variant> &records);

// ---- nimpress_bgzf.cpp ------------------------------------------------------------------------------------------------
bool inflateAll(const std::string &in, std::string &out);  // gzip / zlib / BGZF (concatenated members), whole buffer

// BGZF random access by virtual offset (compressed block offset << 16 | offset inside the inflated block)
struct BgzfFile {
    ~BgzfFile() {
        if (f) fclose(f);
    }
    bool open(const std::string &path);
    // read n bytes starting at virtual offset *voff (advances it); false at EOF / on a short read
    bool readBytes(uint64_t *voff, void *dst, size_t n);
    // read one text line starting at virtual offset *voff (advances it); false at EOF (a last unterminated line is read)
    bool readLine(uint64_t *voff, std::string &line);

private:
    struct At {
        uint64_t coff;
        uint32_t uoff;
    };
    FILE *f = nullptr;
    std::unordered_map<uint64_t, std::pair<std::string, uint32_t>> cache;  // inflated blocks by offset: data, compressed size
    bool block(uint64_t coff, const std::string **data, uint32_t *csize);
    bool advance(At &a, const std::string &d, uint32_t csize);
};

// The bin index of tabix (.tbi) and CSI (.csi) files: one binning scheme -- tabix is min_shift 14, depth 5 plus a linear
// index and the contig names.  load() is false when the file is absent or of another kind and throws on a truncated one.
struct BinIndex {
    typedef std::vector<std::pair<uint64_t, uint64_t>> Chunks;  // virtual offset ranges
    struct Ref {
        std::unordered_map<uint32_t, Chunks> bins;
        std::vector<uint64_t> linear;  // tabix only
    };
    bool tabix = false;
    int32_t min_shift = 14, depth = 5;
    std::vector<Ref> refs;
    std::vector<std::string> names;  // tabix only: the contig of refs[k] (a CSI's contigs are the BCF header's)
    bool load(const std::string &path, bool is_tabix);
    // chunks that may hold records of contig `ref` overlapping [beg0, end0) (0-based), sorted
    Chunks query(size_t ref, int64_t beg0, int64_t end0) const;
};

// ---- nimpress_bcf.cpp -------------------------------------------------------------------------------------------------
struct BcfHeader {
    std::vector<std::string> contigs;  // BCF_DT_CTG
    std::vector<std::string> ids;      // BCF_DT_ID: FILTER/INFO/FORMAT ids, PASS = 0
    std::vector<std::string> samples;
    void parse(const std::string &text);
};
// the fixed 24 bytes a record's shared block starts with
struct BcfHead {
    int32_t chrom, pos0, rlen;
    uint32_t n_allele, n_fmt, n_sample;
};
inline BcfHead bcfRecordHead(const unsigned char *p) {
    BcfHead h;
    uint32_t nai, nfs;
    memcpy(&h.chrom, p, 4);
    memcpy(&h.pos0, p + 4, 4);
    memcpy(&h.rlen, p + 8, 4);
    memcpy(&nai, p + 16, 4);
    memcpy(&nfs, p + 20, 4);
    h.n_allele = nai >> 16;
    h.n_fmt = nfs >> 24;
    h.n_sample = nfs & 0xffffff;
    return h;
}
// one record (shared + indiv blocks, without the two length words) -> Variant; false when `wanted` is given and the
// record overlaps none of its regions (nothing else is decoded then)
bool parseBcfRecord(const unsigned char *shared, size_t l_shared, const unsigned char *indiv, size_t l_indiv,
                    const BcfHeader &h, const RegionMap *wanted, Format prefer, Variant &v);
// whole-file scan of an inflated BCF
void scanBcf(const std::string &text, const RegionMap *wanted, std::vector<std::string> &samples,
             std::vector<Variant> &records);

// ---- nimpress_plink.cpp -----------------------------------------------------------------------------------------------
// PLINK 1 fileset: <prefix>.bed + .bim + .fam, or PLINK 2: .pgen + .pvar + .psam.  False when `path` is neither.
bool openPlinkFileset(const std::string &path, const RegionMap *wanted, std::vector<std::string> &samples,
                      std::vector<Variant> &records);

}  // namespace nimpress
#pragma GCC visibility pop
