// nimpress_bcf.cpp -- see nimpress_readers.hpp.  BCF2 (htslib's binary VCF): header dictionaries + record decoding.
// Layout restated from the VCF/BCF specification (hts-specs VCFv4.3 section 6; the reference reads
// BCF through htslib 1.10.2, Dockerfile:32).  Only what the path needs is decoded: CHROM, POS, ID,
// alleles, FILTER and the FORMAT/GT, /DS and /PL vectors, which are kept in the file's own width.
#include "nimpress_readers.hpp"

#include <algorithm>
#include <cstdlib>

namespace nimpress {
namespace {

// value of key= inside <...> of a header line, honouring quotes
bool attr(const std::string &line, const char *key, std::string &out) {
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

// A FORMAT field as the record holds it, remembered only: whether the record is scored from GT, DS or PL is decided once
// all are seen, and a field that is not used is neither validated nor copied (a file with an oddly typed DS next to its
// GT scores as before).
struct BcfField {
    bool present = false;
    int type = 0;
    int64_t len = 0;  // values per sample
    const unsigned char *ptr = nullptr;
    size_t bytes = 0;
};

}  // namespace

void BcfHeader::parse(const std::string &text) {
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
            sampleNames(line, samples);
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

bool parseBcfRecord(const unsigned char *shared, size_t l_shared, const unsigned char *indiv, size_t l_indiv,
                    const BcfHeader &h, const RegionMap *wanted, Format prefer, Variant &v) {
    BcfCursor c{shared, shared + l_shared};
    c.need(24);
    const BcfHead head = bcfRecordHead(c.p);
    c.p += 24;
    const uint32_t n_sample = head.n_sample;
    if (head.chrom < 0 || (size_t)head.chrom >= h.contigs.size()) throw std::runtime_error("BCF: CHROM out of range");
    v = Variant();
    v.contig = h.contigs[(size_t)head.chrom];
    v.pos = (int64_t)head.pos0 + 1;
    // by the record's own span (POS .. POS + rlen - 1), before anything is copied
    if (wanted && !overlapsWanted(*wanted, v.contig, v.pos, v.pos + std::max<int64_t>(head.rlen, 1) - 1)) return false;
    v.id = c.str();
    if (v.id.empty()) v.id = ".";
    for (uint32_t k = 0; k < head.n_allele; ++k) {
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
    if (n_sample != h.samples.size()) throw std::runtime_error("BCF: record sample count differs from the header");
    BcfCursor f{indiv, indiv + l_indiv};
    BcfField gt, ds, pl;
    for (uint32_t k = 0; k < head.n_fmt; ++k) {
        const int32_t key = f.typedInt();
        BcfField fld;
        f.desc(fld.type, fld.len);
        fld.present = true;
        fld.ptr = f.p;
        fld.bytes = BcfCursor::sizeOf(fld.type) * (size_t)fld.len * n_sample;
        f.need(fld.bytes);
        f.p += fld.bytes;
        if (key < 0 || (size_t)key >= h.ids.size()) continue;
        const std::string &name = h.ids[(size_t)key];
        if (name == "GT") {
            if (fld.type < 1 || fld.type > 3) throw std::runtime_error("BCF: FORMAT/GT is not an integer vector");
            if (fld.len > 8) throw std::runtime_error("ploidy above 8 is not supported");
            v.ploidy = (int)fld.len;
            v.gt_bytes = (int)BcfCursor::sizeOf(fld.type);
            gt = fld;
        } else if (name == "DS") {
            ds = fld;
        } else if (name == "PL" && prefer == Format::PL) {
            pl = fld;
        }
    }
    // (the rule, with its refusals, only for a record that has samples)
    const std::string at = v.contig + ":" + std::to_string(v.pos);
    const int64_t n_alleles = 1 + (int64_t)v.alt.size();
    const Format from = n_sample ? scoredFrom(prefer, gt.present, ds.present, pl.present, n_alleles, "BCF", at)
                                 : gtOrDs(prefer, gt.present, ds.present);
    v.has_gt = v.has_ds = false;  // one of the three is kept
    if (from == Format::PL) {
        const int64_t G = n_alleles * (n_alleles + 1) / 2;
        if (pl.type < 1 || pl.type > 3) throw std::runtime_error("BCF: FORMAT/PL is not an int8, int16 or int32 vector at " + at);
        if (pl.len != G)
            throw std::runtime_error("BCF: FORMAT/PL holds " + std::to_string(pl.len) + " values per sample, " +
                                     std::to_string(G) + " expected for " + std::to_string(n_alleles) + " alleles at " + at);
        v.has_pl = true;
        v.pl_per_sample = (int)pl.len;
        v.pl_bytes = (int)BcfCursor::sizeOf(pl.type);
        v.pl_raw.assign(pl.ptr, pl.ptr + pl.bytes);
    } else if (from == Format::DS) {
        // typed float vector: len values per sample, missing 0x7F800001, end of vector 0x7F800002
        if (ds.type != 5) throw std::runtime_error("BCF: FORMAT/DS is not a float vector");
        if (ds.len < 1) throw std::runtime_error("BCF: empty FORMAT/DS vector");
        v.has_ds = true;
        v.ds_per_sample = (int)ds.len;
        v.ds.resize((size_t)ds.len * n_sample);
        memcpy(v.ds.data(), ds.ptr, ds.bytes);
        for (const float x : v.ds)  // (NaN patterns = missing / end of vector; any finite value is scored: see the text reader)
            if (isInfiniteDs(x)) throw std::runtime_error("FORMAT/DS value " + std::to_string(x) + " is not finite at " + at);
    } else if (gt.present) {
        v.has_gt = true;
        v.gt_raw.assign(gt.ptr, gt.ptr + gt.bytes);
    }
    return true;
}

void scanBcf(const std::string &text, const RegionMap *wanted, std::vector<std::string> &samples,
             std::vector<Variant> &records) {
    const Format prefer = preferredFormat();
    const unsigned char *base = (const unsigned char *)text.data();
    if (text.size() < 9 || memcmp(base, "BCF\2", 4) != 0) throw std::runtime_error("not a BCF2 file");
    uint32_t l_text;
    memcpy(&l_text, base + 5, 4);
    if (9 + (size_t)l_text > text.size()) throw std::runtime_error("truncated BCF header");
    BcfHeader h;
    h.parse(std::string((const char *)base + 9, l_text));
    samples = h.samples;
    size_t o = 9 + (size_t)l_text;
    while (o + 8 <= text.size()) {
        uint32_t ls[2];
        memcpy(ls, base + o, 8);
        o += 8;
        if (o + (size_t)ls[0] + ls[1] > text.size()) throw std::runtime_error("truncated BCF record");
        Variant v;
        if (parseBcfRecord(base + o, ls[0], base + o + ls[0], ls[1], h, wanted, prefer, v))
            records.push_back(std::move(v));
        o += (size_t)ls[0] + ls[1];
    }
}

}  // namespace nimpress
