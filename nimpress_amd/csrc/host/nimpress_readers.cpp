// nimpress_readers.cpp -- see nimpress_host.hpp.  What sits on top of the genotype file reader units (nimpress_readers.hpp):
// the indexed sources with their parallel fetch, VCF::open / openStreaming / fetch, the Variant methods and the record
// lookup (findVariant, RecordIndex).  No libnps symbol is referenced.
#include "nimpress_readers.hpp"

#include <algorithm>
#include <cstdlib>
#include <thread>

namespace nimpress {

const float *Variant::dsRow(int eaidx, size_t n, std::vector<float> &tmp) const {
    if (ds_per_sample == 1 && eaidx <= 1) return ds.data();
    tmp.assign(n, kDsMissing);
    for (size_t i = 0; i < n; ++i) {
        const float *p = &ds[i * (size_t)ds_per_sample];
        if (eaidx >= 1) {
            if (eaidx <= ds_per_sample && !isDsEnd(p[eaidx - 1])) tmp[i] = p[eaidx - 1];
        } else {  // effect allele = REF: 2 - (sum of the ALT dosages); a missing value makes the sample missing
            float sum = 0.0f;
            for (int k = 0; k < ds_per_sample; ++k)
                if (!isDsEnd(p[k])) sum += p[k];
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

// ---- indexed sources: vcf.gz + .tbi and BCF + .csi ------------------------------------------------
// What hts-nim's vcf.query() (nim:358) needs: the header and the index.  Records are fetched per set
// of score rows; every fetching thread inflates through a BGZF handle of its own.
struct __attribute__((visibility("hidden"))) IndexedSource {  // (opaque outside: held through VCF::source only)
    std::string path;
    bool is_bcf = false;
    BcfHeader bcf;
    BinIndex index;
    std::unordered_map<std::string, size_t> contig_id;  // contig -> its number in the index
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

// One record off an index chunk, as far as the fetch loop looks at it before the full parse.  The two file kinds differ in
// how a record is read and peeked: read() is false at the end of the data, sets `skip` for what is no record of the
// row's contig, else the record's start and inclusive end (1-based); parse() is the full parse of the record just read.
struct Peek {
    bool skip;
    int64_t start, last;
};
struct BcfStep {
    const IndexedSource &src;
    BgzfFile &bg;
    Format prefer;
    uint32_t ls[2];
    std::vector<unsigned char> buf;
    bool read(uint64_t *v, const ScoreEntry &, size_t contig, Peek &p) {
        if (!bg.readBytes(v, ls, 8)) return false;
        buf.resize((size_t)ls[0] + ls[1]);
        if (!bg.readBytes(v, buf.data(), buf.size())) throw std::runtime_error("truncated BCF record");
        p.skip = true;
        if (ls[0] < 24) return true;
        const BcfHead h = bcfRecordHead(buf.data());
        if ((size_t)h.chrom != contig) return true;
        p = Peek{false, (int64_t)h.pos0 + 1, (int64_t)h.pos0 + std::max(h.rlen, 1)};
        return true;
    }
    bool parse(const RegionMap &wanted, Variant &var) {
        return parseBcfRecord(buf.data(), ls[0], buf.data() + ls[0], ls[1], src.bcf, &wanted, prefer, var);
    }
};
struct TextStep {
    const IndexedSource &src;
    BgzfFile &bg;
    Format prefer;
    std::string line;
    std::vector<int32_t> tmp;
    bool read(uint64_t *v, const ScoreEntry &e, size_t, Peek &p) {
        if (!bg.readLine(v, line)) return false;
        p.skip = true;
        if (line.empty() || line[0] == '#') return true;
        // cheap pre-check of CHROM and POS before the full parse
        const size_t t1 = line.find('\t');
        const size_t t2 = t1 == std::string::npos ? t1 : line.find('\t', t1 + 1);
        if (t2 == std::string::npos) return true;
        if (line.compare(0, t1, e.contig) != 0) return true;
        const int64_t pos = parseIntNim(line.substr(t1 + 1, t2 - t1 - 1));
        // end of the record: POS + len(REF) - 1 (REF is the fourth column)
        const size_t t3 = line.find('\t', t2 + 1);
        const size_t t4 = t3 == std::string::npos ? t3 : line.find('\t', t3 + 1);
        const int64_t reflen = t4 == std::string::npos ? 1 : (int64_t)(t4 - t3 - 1);
        p = Peek{false, pos, pos + std::max<int64_t>(reflen, 1) - 1};
        return true;
    }
    bool parse(const RegionMap &wanted, Variant &var) {
        return parseRecordLine(line.data(), line.size(), src.n_samples, &wanted, prefer, tmp, var);
    }
};

// records keyed by virtual offset (= file order); a type of this unit, so that no container of it is exported
struct FoundMap : std::map<uint64_t, Variant> {};

// records overlapping entries [first, first+count)
template <class Step>
void fetchRows(const IndexedSource &src, Step &&step, const ScoreEntry *first, size_t count, FoundMap &found) {
    RegionMap wanted;
    for (size_t i = 0; i < count; ++i) wanted[first[i].contig].emplace_back(first[i].pos, first[i].stop());
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
        const auto ci = src.contig_id.find(e.contig);
        if (ci == src.contig_id.end()) continue;
        for (const auto &chunk : src.index.query(ci->second, e.pos - 1, e.stop())) {
            uint64_t v = chunk.first;
            int64_t max_end = 0;
            const auto rs = resume.find(chunk.first);
            if (rs != resume.end() && e.pos > rs->second.max_end) {
                v = rs->second.at;
                max_end = rs->second.max_end;
            }
            while (v < chunk.second) {
                const uint64_t at = v;
                Peek p;
                if (!step.read(&v, e, ci->second, p)) break;
                if (p.skip) continue;
                if (p.start > e.stop()) {  // records are position sorted inside a contig
                    resume[chunk.first] = Resume{at, max_end};
                    break;
                }
                max_end = std::max(max_end, p.last);
                if (found.count(at)) continue;
                Variant var;
                if (step.parse(wanted, var)) found.emplace(at, std::move(var));
            }
        }
    }
}

void fetchRange(const IndexedSource &src, const ScoreEntry *first, size_t count, FoundMap &found) {
    BgzfFile bg;
    if (!bg.open(src.path)) throw std::runtime_error("cannot open " + src.path);
    if (src.is_bcf)
        fetchRows(src, BcfStep{src, bg, preferredFormat(), {0, 0}, {}}, first, count, found);
    else
        fetchRows(src, TextStep{src, bg, preferredFormat(), {}, {}}, first, count, found);
}

std::vector<Variant> fetchParallel(const IndexedSource &src, const ScoreEntry *first, size_t count) {
    Tick tick(timings().inflate_parse);
    const unsigned nt = hostThreads(count);
    std::vector<FoundMap> parts(nt);
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
    FoundMap &all = parts[0];
    for (unsigned t = 1; t < nt; ++t)
        for (auto &kv : parts[t]) all.emplace(kv.first, std::move(kv.second));  // duplicates: first wins
    std::vector<Variant> out;
    out.reserve(all.size());
    for (auto &kv : all) out.push_back(std::move(kv.second));
    return out;
}

// header + index of an indexed file, or null
std::shared_ptr<IndexedSource> openIndexed(const std::string &path, std::vector<std::string> &samples) {
    if (getenv("NIMPRESS_NO_INDEX")) return nullptr;
    auto src = std::make_shared<IndexedSource>();
    src->path = path;
    {  // BCF + CSI
        BgzfFile bg;
        if (bg.open(path)) {
            uint64_t voff = 0;
            unsigned char magic[9];
            if (bg.readBytes(&voff, magic, 9) && memcmp(magic, "BCF\2", 4) == 0 && src->index.load(path + ".csi", false)) {
                uint32_t l_text;
                memcpy(&l_text, magic + 5, 4);
                std::string text(l_text, '\0');
                if (!bg.readBytes(&voff, &text[0], l_text)) throw std::runtime_error("truncated BCF header");
                src->bcf.parse(text);
                src->is_bcf = true;
                samples = src->bcf.samples;
                for (size_t k = 0; k < src->bcf.contigs.size(); ++k) src->contig_id[src->bcf.contigs[k]] = k;
                src->n_samples = samples.size();
                return src;
            }
        }
    }
    {  // vcf.gz + tabix
        BgzfFile bg;
        if (src->index.load(path + ".tbi", true) && bg.open(path)) {
            for (size_t k = 0; k < src->index.names.size(); ++k) src->contig_id[src->index.names[k]] = k;
            uint64_t voff = 0;
            std::string line;
            while (bg.readLine(&voff, line)) {  // header lines
                if (line.empty()) continue;
                if (line[0] != '#') break;
                if (line.compare(0, 6, "#CHROM") == 0) {
                    samples.clear();
                    sampleNames(line, samples);
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

// open(): text VCF (plain or gzip/BGZF), BCF or a PLINK fileset.  With `keep` and an index next to a BGZF file
// (path + ".tbi" / ".csi") only the index chunks overlapping the score loci are inflated -- the random
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
