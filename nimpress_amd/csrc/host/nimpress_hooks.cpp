// nimpress_hooks.cpp -- the nh_* C hooks of libnimpress_host.so: the whole runs nimpress_amd/host.py drives, and the
// pieces of the host logic the Python tests look at one by one (no GPU needed except nh_compute*).
#include "nimpress_internal.hpp"

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <thread>

using namespace nimpress;

extern "C" {

static thread_local std::string g_nh_error;
const char *nh_last_error(void) { return g_nh_error.c_str(); }

// parse a score file: returns number of entries or -1; fills offset; arrays (if non-null) sized cap
long nh_score_parse(const char *path, double *offset, long cap, long *pos, double *beta, double *eaf,
                    int *ref_is_effect, char *text_out, long text_cap) {
    try {
        ScoreFile sf;
        if (!sf.open(path)) {
            g_nh_error = "cannot open";
            return -1;
        }
        if (offset) *offset = sf.offset;
        std::string text = sf.name + "\n" + sf.desc + "\n" + sf.cite + "\n" + sf.genomever + "\n";
        for (size_t i = 0; i < sf.entries.size(); ++i) {
            const ScoreEntry &e = sf.entries[i];
            if ((long)i < cap) {
                if (pos) pos[i] = e.pos;
                if (beta) beta[i] = e.beta;
                if (eaf) eaf[i] = e.eaf;
                if (ref_is_effect) ref_is_effect[i] = e.refseq == e.easeq;
            }
            text += e.contig + "\t" + e.refseq + "\t" + e.easeq + "\n";
        }
        if (text_out && text_cap > 0) {
            strncpy(text_out, text.c_str(), (size_t)text_cap - 1);
            text_out[text_cap - 1] = 0;
        }
        return (long)sf.entries.size();
    } catch (const std::exception &ex) {
        g_nh_error = ex.what();
        return -2;
    }
}

// coverage of every score entry against a BED: out[i] = 0/1; returns n or <0
long nh_bed_covered(const char *score_path, const char *bed_path, int *out, long cap) {
    try {
        ScoreFile sf;
        GenomeIntervals iv;
        if (!sf.open(score_path) || !loadBedIntervals(iv, bed_path)) {
            g_nh_error = "cannot open";
            return -1;
        }
        for (size_t i = 0; i < sf.entries.size() && (long)i < cap; ++i)
            out[i] = isVariantCovered(sf.entries[i], iv, nullptr) ? 1 : 0;
        return (long)sf.entries.size();
    } catch (const std::exception &ex) {
        g_nh_error = ex.what();
        return -2;
    }
}

// VCF: number of samples / records, and per score entry the found record index (or -1), its eaidx
// and its GT buffer (flattened, ploidy returned)
struct nh_vcf {
    VCF vcf;
};
void *nh_vcf_open(const char *path, const char *score_path_or_null) {
    try {
        nh_vcf *h = new nh_vcf;
        ScoreFile sf;
        const std::vector<ScoreEntry> *keep = nullptr;
        if (score_path_or_null && sf.open(score_path_or_null)) keep = &sf.entries;
        if (!h->vcf.open(path, keep)) {
            delete h;
            g_nh_error = "cannot open";
            return nullptr;
        }
        return h;
    } catch (const std::exception &ex) {
        g_nh_error = ex.what();
        return nullptr;
    }
}
// indexed file opened for streaming, then the records of the score's rows fetched window by window
// (what computePolygenicScores does) and kept: the result must equal nh_vcf_open(path, score)
void *nh_vcf_open_streaming(const char *path, const char *score_path, long window) {
    try {
        nh_vcf *h = new nh_vcf;
        ScoreFile sf;
        if (!sf.open(score_path) || !h->vcf.openStreaming(path)) {
            delete h;
            g_nh_error = "cannot open (no index?)";
            return nullptr;
        }
        std::map<std::pair<std::string, int64_t>, Variant> all;  // windows may fetch a record twice
        std::vector<std::pair<std::string, int64_t>> order;
        const size_t w = window > 0 ? (size_t)window : sf.entries.size();
        for (size_t a = 0; a < sf.entries.size(); a += w) {
            const size_t b = std::min(sf.entries.size(), a + w);
            for (Variant &v : h->vcf.fetch(sf.entries.data() + a, b - a)) {
                const auto key = std::make_pair(v.contig + ":" + v.ref + ":" + (v.alt.empty() ? "" : v.alt[0]), v.pos);
                if (all.emplace(key, std::move(v)).second) order.push_back(key);
            }
        }
        for (const auto &k : order) h->vcf.records.push_back(std::move(all[k]));
        return h;
    } catch (const std::exception &ex) {
        g_nh_error = ex.what();
        return nullptr;
    }
}
// header (sample names) only: indexed files keep just header + index, others are read without keeping
// a record
void *nh_vcf_open_header(const char *path) {
    try {
        nh_vcf *h = new nh_vcf;
        const std::vector<ScoreEntry> none;
        if (!h->vcf.openStreaming(path) && !h->vcf.open(path, &none)) {
            delete h;
            g_nh_error = "cannot open";
            return nullptr;
        }
        return h;
    } catch (const std::exception &ex) {
        g_nh_error = ex.what();
        return nullptr;
    }
}
void nh_vcf_close(void *h) { delete (nh_vcf *)h; }
long nh_vcf_n_samples(void *h) { return (long)((nh_vcf *)h)->vcf.samples.size(); }
int nh_vcf_indexed(void *h) { return ((nh_vcf *)h)->vcf.indexed ? 1 : 0; }
long nh_vcf_n_records(void *h) { return (long)((nh_vcf *)h)->vcf.records.size(); }
const char *nh_vcf_sample(void *h, long i) { return ((nh_vcf *)h)->vcf.samples[(size_t)i].c_str(); }
// all sample names, '\n'-separated, in one call (half a million ctypes calls cost a tenth of a second): returns the
// number of bytes needed (without the terminator); copies when cap is large enough
long nh_vcf_samples_joined(void *h, char *out, long cap) {
    const std::vector<std::string> &s = ((nh_vcf *)h)->vcf.samples;
    size_t need = 0;
    for (const std::string &x : s) need += x.size() + 1;
    if (need) --need;
    if (out && (long)need < cap) {
        char *p = out;
        for (size_t i = 0; i < s.size(); ++i) {
            if (i) *p++ = '\n';
            memcpy(p, s[i].data(), s[i].size());
            p += s[i].size();
        }
        *p = 0;
    }
    return (long)need;
}
// returns record index or -1; fills pos, ploidy, filter (copied), gts (cap int32)
long nh_vcf_find(void *h, const char *contig, long pos, const char *ref, const char *ea, long *rec_pos,
                 int *ploidy, char *filter, long filter_cap, int *gts, long gts_cap) {
    const VCF &vcf = ((nh_vcf *)h)->vcf;
    const Variant *v = findVariant(contig, pos, ref, ea, vcf);
    {  // the indexed lookup the score driver uses must give the same record
        RecordIndex idx;
        idx.build(vcf.records);
        if (idx.find(contig, pos, ref, ea) != v) {
            g_nh_error = "RecordIndex::find disagrees with findVariant";
            return -99;
        }
    }
    if (!v) return -1;
    if (rec_pos) *rec_pos = v->pos;
    if (ploidy) *ploidy = v->ploidy;
    if (filter && filter_cap > 0) {
        strncpy(filter, v->filter.c_str(), (size_t)filter_cap - 1);
        filter[filter_cap - 1] = 0;
    }
    const size_t nval = v->is_bed || v->is_pgen ? 2 * vcf.samples.size()
                        : v->gt_raw.empty() ? v->gts.size() : v->gt_raw.size() / (size_t)v->gt_bytes;
    for (size_t i = 0; i < nval && (long)i < gts_cap; ++i) gts[i] = v->gtValue(i);
    return (long)(v - vcf.records.data());
}

// the FORMAT/DS row the score loop would push for this score row (see Variant::dsRow): returns the number of
// values written (= samples), 0 when the record found is scored from GT, -1 when no record matches
long nh_vcf_find_ds(void *h, const char *contig, long pos, const char *ref, const char *ea, float *out, long cap) {
    const VCF &vcf = ((nh_vcf *)h)->vcf;
    const Variant *v = findVariant(contig, pos, ref, ea, vcf);
    if (!v) return -1;
    if (!v->has_ds) return 0;
    int eaidx = 0;
    if (std::string(ref) != ea) {
        eaidx = -1;
        for (size_t k = 0; k < v->alt.size(); ++k)
            if (v->alt[k] == ea) eaidx = (int)k + 1;
    }
    std::vector<float> tmp;
    const float *row = v->dsRow(eaidx, vcf.samples.size(), tmp);
    const long n = std::min<long>((long)vcf.samples.size(), cap);
    memcpy(out, row, sizeof(float) * (size_t)n);
    return n;
}

// the FORMAT/PL row the score loop would score for this score row (decodePlDosage of the record's vector, the host mirror of
// the device decode): returns the number of values written (= samples), 0 when the record found is not scored from PL
// (NIMPRESS_FORMAT=PL unset, no PL, or more than 8 alleles), -1 when no record matches, -2 on error (nh_last_error)
long nh_vcf_find_pl(void *h, const char *contig, long pos, const char *ref, const char *ea, float *out, long cap) {
    try {
        const VCF &vcf = ((nh_vcf *)h)->vcf;
        const Variant *v = findVariant(contig, pos, ref, ea, vcf);
        if (!v) return -1;
        if (!v->has_pl) return 0;
        int eaidx = 0;
        if (std::string(ref) != ea) {
            eaidx = -1;
            for (size_t k = 0; k < v->alt.size(); ++k)
                if (v->alt[k] == ea) eaidx = (int)k + 1;
        }
        std::vector<float> row(vcf.samples.size());
        decodePlDosage(v->pl_raw.data(), v->pl_bytes, row.size(), 1 + (int)v->alt.size(), eaidx, row.data());
        const long n = std::min<long>((long)row.size(), cap);
        if (n > 0) memcpy(out, row.data(), sizeof(float) * (size_t)n);
        return n;
    } catch (const std::exception &ex) {
        g_nh_error = ex.what();
        return -2;
    }
}

// The row classifier both scoring drivers call (classifyRow), for every row of a score file against a genotype file
// opened with the score loci kept, with an optional coverage BED: kind (0 = genotyped, else nps_row_kind), eaidx,
// ref_is_effect and code map per row (cap ints each), the FILTER strings of the rows '\n'-joined.  Returns the
// number of rows, < 0 on error.
long nh_classify(const char *score_path, const char *vcf_path, const char *bed_path_or_null, int ignorefilt, long cap,
                 int *kind, int *eaidx, int *ref_is_effect, int *code_map, char *filters_out, long filters_cap) {
    try {
        ScoreFile sf;
        VCF vcf;
        GenomeIntervals cov;
        if (!sf.open(score_path) || !vcf.open(vcf_path, &sf.entries) ||
            (bed_path_or_null && !loadBedIntervals(cov, bed_path_or_null))) {
            g_nh_error = "cannot open";
            return -1;
        }
        RecordIndex index;
        index.build(vcf.records);
        std::string filters;
        for (size_t i = 0; i < sf.entries.size() && (long)i < cap; ++i) {
            const RowClass c = classifyRow(sf.entries[i], bed_path_or_null != nullptr, cov, index, ignorefilt != 0);
            kind[i] = c.kind, eaidx[i] = c.eaidx, ref_is_effect[i] = c.ref_is_effect, code_map[i] = c.code_map;
            filters += c.filter + "\n";
        }
        if (filters_out && filters_cap > 0) {
            strncpy(filters_out, filters.c_str(), (size_t)filters_cap - 1);
            filters_out[filters_cap - 1] = 0;
        }
        return (long)sf.entries.size();
    } catch (const std::exception &ex) {
        g_nh_error = ex.what();
        return -2;
    }
}

// The warning writer both scoring drivers call (writeRowWarnings), for one row: its log lines ("WARN ...") go to
// out, '\n'-terminated.  Returns their number, < 0 on error (-1: out is too small).
long nh_row_warnings(const char *contig, long pos, const char *ref, const char *ea, double eaf, int kind, const char *filter,
                     const char *pre_warning, long nsamples, long nmissing, double neffect, int over_maxmis, double afmisp,
                     char *out, long cap) {
    try {
        ScoreEntry e;
        e.contig = contig, e.pos = pos, e.refseq = ref, e.easeq = ea, e.eaf = eaf;
        Log log;
        log.echo = false;
        writeRowWarnings(log, e, kind, filter, pre_warning, nsamples, (uint64_t)nmissing, neffect, over_maxmis != 0, afmisp);
        std::string all;
        for (const std::string &l : log.lines) all += l + "\n";
        if ((long)all.size() >= cap) {
            g_nh_error = "nh_row_warnings: out is too small";
            return -1;
        }
        memcpy(out, all.c_str(), all.size() + 1);
        return (long)log.lines.size();
    } catch (const std::exception &ex) {
        g_nh_error = ex.what();
        return -2;
    }
}

// whole run (needs a GPU): the reference's main() minus printing.  Returns the number of samples,
// or < 0 on error (nh_last_error).  scores_out has room for cap doubles; warnings (newline separated)
// go to log_out.
// the complete log text of the last nh_compute* call of this thread (the caller's log_out buffer may have been too
// small for it: it then ends at a line end followed by "... log truncated"), and the time breakdown of that call
static thread_local std::string g_nh_log;
long nh_last_log_size() { return (long)g_nh_log.size(); }
long nh_last_log(char *out, long cap) {
    if (!out || cap <= 0) return -1;
    const size_t n = std::min(g_nh_log.size(), (size_t)cap - 1);
    memcpy(out, g_nh_log.data(), n);
    out[n] = 0;
    return (long)n;
}
static void copyLog(const std::string &all, char *log_out, long log_cap) {
    g_nh_log = all;
    if (!log_out || log_cap <= 0) return;
    if ((long)all.size() < log_cap) {
        memcpy(log_out, all.c_str(), all.size() + 1);
        return;
    }
    // too small: whole lines only, and say so (nh_last_log has the full text)
    static const char kMark[] = "... log truncated\n";
    size_t room = (size_t)log_cap - 1 > sizeof kMark - 1 ? (size_t)log_cap - 1 - (sizeof kMark - 1) : 0;
    size_t cut = all.rfind('\n', room ? room - 1 : 0);
    cut = cut == std::string::npos || room == 0 ? 0 : cut + 1;
    memcpy(log_out, all.data(), cut);
    const size_t m = std::min(sizeof kMark - 1, (size_t)log_cap - 1 - cut);
    memcpy(log_out + cut, kMark, m);
    log_out[cut + m] = 0;
}
// out[0..6] = hip_init, hip_init_wait, open, inflate_parse, push, kernels, warnings (seconds) of the last nh_compute* call
void nh_last_timings(double *out7) {
    const Timings &t = timings();
    out7[0] = t.hip_init, out7[1] = t.hip_init_wait, out7[2] = t.open, out7[3] = t.inflate_parse, out7[4] = t.push,
    out7[5] = t.kernels, out7[6] = t.warnings;
}

// What both whole-run hooks do before they score: the HIP context comes up on its own thread (joined on every way
// out) while the score files, the genotype file -- for streaming if asked and possible, else with the score loci kept
// -- and the coverage BED are opened.
namespace {
struct RunInputs {
    struct Join {
        ~Join() { warmupJoin(); }
    } join_on_exit;  // (first member: destroyed last)
    std::vector<ScoreFile> files;
    VCF vcf;
    GenomeIntervals cov;
    bool restrict = false;
    std::string bed_error;  // the run goes on without the BED, as the reference's does: a FATAL line of the log
    // false with the message in g_nh_error
    bool open(const std::vector<std::string> &score_paths, const char *vcf_path, const char *bed_path_or_null, int device,
              bool stream) {
        timingsReset();
        warmupStart(device);  // the HIP context comes up while the files are opened, inflated and parsed
        const double t0 = nowSeconds();
        files.resize(score_paths.size());
        std::vector<ScoreEntry> all;  // (several files: the loci of all of them are kept)
        for (size_t i = 0; i < files.size(); ++i) {
            if (!files[i].open(score_paths[i])) {
                g_nh_error = "Could not open polygenic score file " + score_paths[i];
                return false;
            }
            if (files.size() > 1) all.insert(all.end(), files[i].entries.begin(), files[i].entries.end());
        }
        const std::vector<ScoreEntry> &keep = files.size() == 1 ? files[0].entries : all;
        if (!((stream && vcf.openStreaming(vcf_path)) || vcf.open(vcf_path, &keep))) {
            g_nh_error = std::string("Could not open input VCF file ") + vcf_path;
            return false;
        }
        timings().open += nowSeconds() - t0 - timings().inflate_parse;
        restrict = bed_path_or_null != nullptr;
        if (restrict && !loadBedIntervals(cov, bed_path_or_null))
            bed_error = std::string("Could not open coverage BED file ") + bed_path_or_null;
        return true;
    }
};
}  // namespace

static long nh_compute_impl(const char *score_path, const char *vcf_path, const char *bed_path_or_null,
                            int imp_locus, int imp_missing, int imp_sample, double maxmis, double afmisp,
                            long mincs, int ignorefilt, int device, double *scores_out, long cap, double *d_scores_out,
                            unsigned long long *nloci_out, char *log_out, long log_cap) {
    try {
        RunInputs in;
        // (the command line always streams)
        if (!in.open({score_path}, vcf_path, bed_path_or_null, device, getenv("NIMPRESS_STREAM") != nullptr)) return -1;
        Log log;
        log.echo = false;
        if (!in.bed_error.empty()) log.fatal(in.bed_error);
        std::vector<double> scores;
        uint64_t nloci = 0;
        computePolygenicScores(scores, in.files[0], in.vcf, in.restrict, in.cov, (ImputeMethodLocus)imp_locus,
                               (ImputeMethodMissing)imp_missing, (ImputeMethodSample)imp_sample, maxmis,
                               afmisp, mincs, ignorefilt != 0, log, device, &nloci, d_scores_out);
        if (nloci_out) *nloci_out = nloci;
        for (size_t i = 0; i < scores.size() && (long)i < cap; ++i) scores_out[i] = scores[i];
        std::string all;
        for (const std::string &l : log.lines) all += l + "\n";
        copyLog(all, log_out, log_cap);
        return (long)in.vcf.n_samples();
    } catch (const std::exception &ex) {
        g_nh_error = ex.what();
        return -2;
    }
}

long nh_compute(const char *score_path, const char *vcf_path, const char *bed_path_or_null,
                int imp_locus, int imp_missing, int imp_sample, double maxmis, double afmisp,
                long mincs, int ignorefilt, int device, double *scores_out, long cap,
                unsigned long long *nloci_out, char *log_out, long log_cap) {
    return nh_compute_impl(score_path, vcf_path, bed_path_or_null, imp_locus, imp_missing, imp_sample, maxmis, afmisp, mincs,
                           ignorefilt, device, scores_out, cap, nullptr, nloci_out, log_out, log_cap);
}
// the same with the n_samples scores left in DEVICE memory (d_scores_out; nps_finish_device): no host bounce before a
// multi-GPU gather
long nh_compute_dev(const char *score_path, const char *vcf_path, const char *bed_path_or_null,
                    int imp_locus, int imp_missing, int imp_sample, double maxmis, double afmisp,
                    long mincs, int ignorefilt, int device, void *d_scores_out,
                    unsigned long long *nloci_out, char *log_out, long log_cap) {
    if (!d_scores_out) {
        g_nh_error = "nh_compute_dev: d_scores_out is NULL";
        return -1;
    }
    return nh_compute_impl(score_path, vcf_path, bed_path_or_null, imp_locus, imp_missing, imp_sample, maxmis, afmisp, mincs,
                           ignorefilt, device, nullptr, 0, (double *)d_scores_out, nloci_out, log_out, log_cap);
}

// S score files on one genotype file in ONE pass over the genotypes (computePolygenicScoresMulti).  score_paths:
// newline-separated.  scores_out: [S][n] doubles (cap = room per file); log lines come back prefixed "<file index>\t".
// Returns the number of samples, < 0 on error.
static long nh_compute_multi_impl(const char *score_paths, const char *vcf_path, const char *bed_path_or_null, int imp_locus,
                                  int imp_missing, int imp_sample, double maxmis, double afmisp, long mincs, int ignorefilt,
                                  int device, int shard, int n_shards, bool partial, double *scores_out, long cap,
                                  unsigned long long *nloci_out, double *offsets_out, char *log_out, long log_cap,
                                  double *d_out = nullptr, bool accept_ds = false) {
    try {
        RunInputs in;
        // (a shard of the rows reads only its own records: an indexed file is opened for window-by-window fetches,
        // which computePolygenicScoresMulti asks for its block alone)
        if (!in.open(splitChar(score_paths, '\n'), vcf_path, bed_path_or_null, device,
                     getenv("NIMPRESS_STREAM") != nullptr || n_shards > 1))
            return -1;
        std::vector<const ScoreFile *> ptrs;
        for (size_t i = 0; i < in.files.size(); ++i) {
            ptrs.push_back(&in.files[i]);
            if (offsets_out) offsets_out[i] = in.files[i].offset;
        }
        std::vector<Log> logs;
        const std::string pre = in.bed_error.empty() ? "" : "FATAL " + in.bed_error;
        std::vector<std::vector<double>> scores;
        std::vector<uint64_t> nloci;
        computePolygenicScoresMulti(scores, ptrs, in.vcf, in.restrict, in.cov, (ImputeMethodLocus)imp_locus,
                                    (ImputeMethodMissing)imp_missing, (ImputeMethodSample)imp_sample, maxmis, afmisp, mincs,
                                    ignorefilt != 0, logs, device, &nloci, shard, n_shards, partial, d_out, accept_ds);
        for (size_t s = 0; s < scores.size(); ++s) {
            for (size_t i = 0; i < scores[s].size() && (long)i < cap; ++i) scores_out[s * (size_t)cap + i] = scores[s][i];
            if (nloci_out) nloci_out[s] = nloci[s];
        }
        std::string allt;
        for (size_t s = 0; s < logs.size(); ++s) {
            if (!pre.empty()) allt += std::to_string(s) + "\t" + pre + "\n";
            for (const std::string &l : logs[s].lines) allt += std::to_string(s) + "\t" + l + "\n";
        }
        copyLog(allt, log_out, log_cap);  // (every line carries its file index: a cut at a line end keeps them apart)
        return (long)in.vcf.n_samples();
    } catch (const std::exception &ex) {
        g_nh_error = ex.what();
        return -2;
    }
}

long nh_compute_multi(const char *score_paths, const char *vcf_path, const char *bed_path_or_null, int imp_locus,
                      int imp_missing, int imp_sample, double maxmis, double afmisp, long mincs, int ignorefilt,
                      int device, double *scores_out, long cap, unsigned long long *nloci_out, char *log_out,
                      long log_cap) {
    return nh_compute_multi_impl(score_paths, vcf_path, bed_path_or_null, imp_locus, imp_missing, imp_sample, maxmis, afmisp,
                                 mincs, ignorefilt, device, 0, 1, false, scores_out, cap, nloci_out, nullptr, log_out,
                                 log_cap);
}

// Block `shard` of n_shards of the union's rows, ALL files, before the normalisation: sums_out [S][cap] un-normalised
// sums, nloci_out [S] the block's counts, offsets_out [S] the files' offsets (computePolygenicScoresMulti with
// partial = true: the rows-sharded x all-scores layout; the caller sum-all-reduces sums and nloci over the shards and
// applies sums / (2 nloci) + offset).
long nh_compute_multi_partial(const char *score_paths, const char *vcf_path, const char *bed_path_or_null, int imp_locus,
                              int imp_missing, int imp_sample, double maxmis, double afmisp, long mincs, int ignorefilt,
                              int device, int shard, int n_shards, double *sums_out, long cap,
                              unsigned long long *nloci_out, double *offsets_out, char *log_out, long log_cap) {
    return nh_compute_multi_impl(score_paths, vcf_path, bed_path_or_null, imp_locus, imp_missing, imp_sample, maxmis, afmisp,
                                 mincs, ignorefilt, device, shard, n_shards, true, sums_out, cap, nloci_out, offsets_out,
                                 log_out, log_cap);
}

// the two above with the results left in DEVICE memory: d_out = [S][n_samples] doubles (scores, or with n_shards > 1
// the block's un-normalised sums for the all-reduce): nps_multi_finish_device / nps_multi_partial_device
long nh_compute_multi_dev(const char *score_paths, const char *vcf_path, const char *bed_path_or_null, int imp_locus,
                          int imp_missing, int imp_sample, double maxmis, double afmisp, long mincs, int ignorefilt,
                          int device, int shard, int n_shards, int partial, void *d_out, unsigned long long *nloci_out,
                          double *offsets_out, char *log_out, long log_cap) {
    if (!d_out) {
        g_nh_error = "nh_compute_multi_dev: d_out is NULL";
        return -1;
    }
    return nh_compute_multi_impl(score_paths, vcf_path, bed_path_or_null, imp_locus, imp_missing, imp_sample, maxmis, afmisp,
                                 mincs, ignorefilt, device, shard, n_shards, partial != 0, nullptr, 0, nloci_out, offsets_out,
                                 log_out, log_cap, (double *)d_out);
}

// The three hooks above in one, with a flags word: bit 0 (host.py: MULTI_ACCEPT_DS) = FORMAT/DS records are scored too
// (computePolygenicScoresMulti's acceptDs).  d_out non-null: results stay on the device (scores_out and cap unused);
// partial: the block's un-normalised sums.
long nh_compute_multi_ex(const char *score_paths, const char *vcf_path, const char *bed_path_or_null, int imp_locus,
                         int imp_missing, int imp_sample, double maxmis, double afmisp, long mincs, int ignorefilt, int device,
                         int shard, int n_shards, int partial, unsigned flags, double *scores_out, long cap, void *d_out,
                         unsigned long long *nloci_out, double *offsets_out, char *log_out, long log_cap) {
    if (!d_out && !scores_out) {
        g_nh_error = "nh_compute_multi_ex: scores_out and d_out are NULL";
        return -1;
    }
    return nh_compute_multi_impl(score_paths, vcf_path, bed_path_or_null, imp_locus, imp_missing, imp_sample, maxmis, afmisp,
                                 mincs, ignorefilt, device, shard, n_shards, partial != 0, d_out ? nullptr : scores_out,
                                 d_out ? 0 : cap, nloci_out, offsets_out, log_out, log_cap, (double *)d_out, (flags & 1u) != 0);
}

// the host's decode of a FORMAT/GT vector (elem_bytes 1 / 2 / 4) and of .bed / .pgen codes into the float32 row of effect
// allele counts the one-pass dosage route uploads (decodeGtDosage, decodeCodeDosage): n values written, -1 on bad arguments
long nh_decode_gt_dosage(const void *gts, int elem_bytes, long n, int ploidy, int eaidx, float *out) {
    if (!gts || !out || n < 0 || ploidy < 1 || (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4)) return -1;
    decodeGtDosage(gts, elem_bytes, (size_t)n, ploidy, eaidx, out);
    return n;
}
// the host's decode of a typed FORMAT/PL vector (decodePlDosage): n values written, -1 on bad arguments
long nh_decode_pl_dosage(const void *pl, int elem_bytes, long n, int n_alleles, int eaidx, float *out) {
    if (!pl || !out || n < 0 || n_alleles < 2 || n_alleles > 8 || eaidx < 0 || eaidx >= n_alleles ||
        (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4))
        return -1;
    try {
        decodePlDosage(pl, elem_bytes, (size_t)n, n_alleles, eaidx, out);
    } catch (const std::exception &ex) {
        g_nh_error = ex.what();
        return -1;
    }
    return n;
}
long nh_decode_code_dosage(const unsigned char *codes, long n, int code_map, float *out) {
    if (!codes || !out || n < 0 || code_map < 0 || code_map > 3) return -1;
    decodeCodeDosage(codes, (size_t)n, code_map, out);
    return n;
}

double nh_dbinom(long x, long n, double p) { return dbinom(x, n, p); }
double nh_pbinom(long x, long n, double p) { return pbinom(x, n, p); }
double nh_binom_test(long x, long n, double p) { return binomTest(x, n, p); }
double nh_binom_test_fast(long x, long n, double p) { return binomTestFast(x, n, p); }
double nh_betai(double a, double b, double x) { return betai(a, b, x); }
void nh_format_float(double x, char *out, long cap) {
    const std::string s = formatFloat(x);
    strncpy(out, s.c_str(), (size_t)cap - 1);
    out[cap - 1] = 0;
}

// The samples x scores matrix of several score files, one line per sample: name TAB score 1 TAB score 2 ..., every
// value as the reference prints a score (nimpress.nim:752-753: formatFloat).  scores = [n_scores][row_stride]
// doubles, names_nl = the n sample names separated by '\n'.  Formatting millions of values is what a multi-file run
// spends its time on once the genotypes are scored in one pass, so the lines are made by up to 16 threads and
// written in order.  path "-" = stdout.  Returns 0, or -1 with the message in nh_last_error().
long nh_write_matrix_tsv(const char *path, const char *names_nl, long n, const double *scores, long n_scores,
                         long row_stride) {
    try {
        if (n < 0 || n_scores < 0 || row_stride < n) throw std::runtime_error("nh_write_matrix_tsv: bad shape");
        std::vector<std::pair<const char *, size_t>> names((size_t)n);
        const char *p = names_nl;
        for (long i = 0; i < n; ++i) {
            const char *q = strchr(p, '\n');
            if (!q) q = p + strlen(p);
            names[(size_t)i] = {p, (size_t)(q - p)};
            p = *q ? q + 1 : q;
        }
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        const long n_thr = std::max<long>(1, std::min<long>({16, (long)hw, n / 2048 + 1}));
        std::vector<std::string> parts((size_t)n_thr);
        std::vector<std::exception_ptr> err((size_t)n_thr);  // (an exception must not leave a worker thread: std::terminate)
        auto work = [&](long t) {
            try {
                const long a = n * t / n_thr, b = n * (t + 1) / n_thr;
                std::string &o = parts[(size_t)t];
                o.reserve((size_t)(b - a) * (size_t)(16 + 24 * n_scores));
                for (long i = a; i < b; ++i) {
                    o.append(names[(size_t)i].first, names[(size_t)i].second);
                    for (long k = 0; k < n_scores; ++k) {
                        char buf[32];
                        o.push_back('\t');
                        o.append(buf, formatFloatTo(scores[k * row_stride + i], buf));
                    }
                    o.push_back('\n');
                }
            } catch (...) {
                err[(size_t)t] = std::current_exception();
            }
        };
        std::vector<std::thread> thr;
        for (long t = 1; t < n_thr; ++t) thr.emplace_back(work, t);
        work(0);
        for (auto &t : thr) t.join();
        for (const std::exception_ptr &e : err)
            if (e) std::rethrow_exception(e);  // the first worker's error, after every thread has been joined
        FILE *f = strcmp(path, "-") == 0 ? stdout : fopen(path, "w");
        if (!f) throw std::runtime_error(std::string("cannot open ") + path + ": " + strerror(errno));
        bool ok = true;
        for (const std::string &o : parts) ok = ok && fwrite(o.data(), 1, o.size(), f) == o.size();
        if (f == stdout)
            ok = fflush(f) == 0 && ok;
        else
            ok = fclose(f) == 0 && ok;
        if (!ok) throw std::runtime_error(std::string("write to ") + path + " failed: " + strerror(errno));
        return 0;
    } catch (const std::exception &e) {
        g_nh_error = e.what();
        return -1;
    }
}

}  // extern "C"
