// nimpress_scoring.cpp -- see nimpress_host.hpp.  The two scoring drivers above the libnps C-ABI: the reference's control
// flow per score row (classifyRow), its warnings (writeRowWarnings), and the HIP context's warm-up thread.  No
// per-sample arithmetic: every located record goes to libnps as it was read.
#include "nimpress_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <thread>

#include "../../../include/nps.h"

namespace nimpress {

// ---- the HIP context on a thread of its own -------------------------------------------------------------
// one warm-up at a time per process (a second caller while one is in flight simply does without: its first libnps
// call creates the context as before)
static std::mutex g_warm_mutex;
static std::thread g_warm_thread;
static std::thread::id g_warm_owner;
// the warm-up thread's elapsed time travels WITH the thread object: each launch has its own slot, moved out together with
// the thread by the one caller that joins it (a shared global was written by a new launch while the previous joiner still
// read it: ADVICE round 4)
static std::shared_ptr<double> g_warm_seconds;
void warmupStart(int device) {
    std::lock_guard<std::mutex> lock(g_warm_mutex);
    if (g_warm_thread.joinable()) return;
    auto slot = std::make_shared<double>(0.0);
    g_warm_seconds = slot;
    g_warm_owner = std::this_thread::get_id();
    g_warm_thread = std::thread([device, slot]() {
        const double t0 = nowSeconds();
        (void)nps_warmup(device);  // (an error shows up again, with its message, in the run's first libnps call)
        *slot = nowSeconds() - t0;  // (read only after join())
    });
}
void warmupJoin() {
    std::thread t;
    std::shared_ptr<double> slot;
    {
        std::lock_guard<std::mutex> lock(g_warm_mutex);
        if (!g_warm_thread.joinable() || g_warm_owner != std::this_thread::get_id()) return;
        t = std::move(g_warm_thread);
        slot = std::move(g_warm_seconds);
    }
    Tick tick(timings().hip_init_wait);
    t.join();
    if (slot) timings().hip_init += *slot;
}

// ------------------------------------------------------------------------------------------
// what both drivers need around the libnps C-ABI
static void npsCheck(int rc, const char *what) {
    if (rc != NPS_OK)
        throw std::runtime_error(std::string(what) + " failed (" + std::to_string(rc) + "): " +
                                 nps_last_error());
}

// one move-only owner per libnps object: released when it goes out of scope, in reverse order of creation
struct NpsRelease {
    void operator()(nps_ctx *x) const { nps_destroy(x); }
    void operator()(nps_cohort *x) const { nps_cohort_destroy(x); }
    void operator()(nps_multidef *x) const { nps_multidef_destroy(x); }
    void operator()(nps_multi *x) const { nps_multi_destroy(x); }
};
template <class T>
using Handle = std::unique_ptr<T, NpsRelease>;
// the object a libnps create call hands out (create: T ** -> status), owned before the status is looked at
template <class T, class Create>
static Handle<T> created(const char *what, Create create) {
    T *raw = nullptr;
    const int rc = create(&raw);
    Handle<T> h(raw);
    npsCheck(rc, what);
    return h;
}

static nps_params makeParams(ImputeMethodLocus imputeMethodLocus, ImputeMethodMissing imputeMethodMissing,
                             ImputeMethodSample imputeMethodSample, double maxMissingRate, int64_t minGtForInternalImput) {
    nps_params p;
    p.imp_locus = (int32_t)imputeMethodLocus;
    p.imp_missing = (int32_t)imputeMethodMissing;
    p.imp_sample = (int32_t)imputeMethodSample;
    p.reserved = 0;
    p.max_missing_rate = maxMissingRate;
    p.min_cs = minGtForInternalImput;
    return p;
}

// Score rows per fetch of a streaming source (an indexed file opened with openStreaming): the records of one window
// of rows are fetched by several threads, pushed, dropped -- so the host holds window x samples genotypes, not
// loci x samples.  512 MiB of diploid int32 rows, at least 64 and at most 8192 rows; NIMPRESS_WINDOW overrides.
static size_t streamingWindow(int64_t nsamples) {
    const size_t per_row = (size_t)std::max<int64_t>(nsamples, 1) * 8;  // diploid int32 at most
    size_t window = std::min<size_t>(std::max<size_t>((512u << 20) / per_row, 64), 8192);
    if (const char *w = getenv("NIMPRESS_WINDOW"))
        if (atoi(w) > 0) window = (size_t)atoi(w);
    return std::max<size_t>(window, 1);
}

// ------------------------------------------------------------------------------------------
// getImputedDosages' control flow (nim:523-585), once for both drivers: the row's class, then its warnings
RowClass classifyRow(const ScoreEntry &e, bool restrictToCoveredRgns, const GenomeIntervals &coveredIvals,
                     const RecordIndex &index, bool ignoreFilterField) {
    RowClass c;
    c.ref_is_effect = e.refseq == e.easeq ? 1 : 0;
    if (restrictToCoveredRgns && !isVariantCovered(e, coveredIvals, &c.pre_warning)) {
        c.kind = NPS_ROW_UNCOVERED;  // nim:526-531
        return c;
    }
    const Variant *v = c.v = index.find(e.contig, e.pos, e.refseq, e.easeq);  // nim:533
    if (!v) {  // nim:536-551
        c.kind = NPS_ROW_ABSENT;
        return c;
    }
    if (!ignoreFilterField && v->filter != "." && v->filter != "PASS") {  // :553
        c.kind = NPS_ROW_FILTERED;
        c.filter = v->filter;
        return c;
    }
    if (!c.ref_is_effect) {  // nim:375-379
        c.eaidx = -1;
        for (size_t k = 0; k < v->alt.size(); ++k)
            if (v->alt[k] == e.easeq) {
                c.eaidx = (int)k + 1;
                break;
            }
    }
    // the code map of a PLINK record's 2-bit codes.  .bed: A1 / A2 (a .bim has no REF); .pgen: REF / ALT
    if (v->is_bed) c.code_map = e.easeq == v->alt[0] ? NPS_MAP_BED_A1 : NPS_MAP_BED_A2;
    if (v->is_pgen) c.code_map = c.eaidx == 0 ? NPS_MAP_PGEN_REF : NPS_MAP_PGEN_ALT;
    if (v->has_ds && v->ds_per_sample == 1 && v->alt.size() > 1 && c.eaidx <= 1)
        c.pre_warning += (c.pre_warning.empty() ? "" : "\n") + std::string("Variant ") + e.contig + ":" +
                         std::to_string(e.pos) + " has one FORMAT/DS value per sample at a site with " +
                         std::to_string(v->alt.size()) + " ALT alleles; it is taken as the dosage of " +
                         "the first ALT allele.";
    return c;
}

void writeRowWarnings(Log &log, const ScoreEntry &e, int kind, const std::string &filter, const std::string &pre_warning,
                      int64_t nsamples, uint64_t nmissing, double neffect, bool over_maxmis, double afMismatchPthresh) {
    const std::string locus = e.contig + ":" + std::to_string(e.pos);
    const std::string var = locus + ":" + e.refseq + ":" + e.easeq;
    if (!pre_warning.empty()) log.warn(pre_warning);
    switch (kind) {
    case NPS_ROW_UNCOVERED:  // nim:527-530
        log.warn("Locus " + locus + "-" + std::to_string(e.stop()) +
                 " is not covered by the sequence coverage BED.  Imputing all dosages at this locus.");
        break;
    case NPS_ROW_ABSENT:  // nim:537-541
        if (!std::isnan(e.eaf) && binomTestFast(0, nsamples * 2, e.eaf) < afMismatchPthresh)
            log.warn("Variant " + var + " cohort EAF is 0 in " + std::to_string(nsamples) +
                     " samples.  This is highly unlikely given polygenic score EAF of " +
                     formatFloat(e.eaf));
        break;
    case NPS_ROW_FILTERED:  // nim:554-557
        log.warn("Variant " + var + " has a FILTER flag set (value \"" + filter +
                 "\").  Imputing all dosages at this locus.");
        break;
    default:
        if (over_maxmis) {  // nim:567-570
            const double missingrate = (double)nmissing / (double)nsamples;
            log.warn("Locus " + locus + "-" + std::to_string(e.stop()) + " has " +
                     formatFloat(missingrate * 100) +
                     "% of samples missing a genotype. This exceeds the missingness threshold; "
                     "imputing all dosages at this locus.");
        } else {  // nim:573-579
            const int64_t nobs = (nsamples - (int64_t)nmissing) * 2;
            if (!std::isnan(e.eaf) &&
                binomTestFast((int64_t)llround(neffect), nobs, e.eaf) < afMismatchPthresh)
                log.warn("Variant " + var + " cohort EAF is " +
                         formatFloat(neffect / (double)nobs) + " in " +
                         std::to_string(nsamples) +
                         " samples.  This is highly unlikely given polygenic score EAF of " +
                         formatFloat(e.eaf));
        }
        break;
    }
}

// ------------------------------------------------------------------------------------------
// getRawDosages on the host (nimpress_internal.hpp)
template <class T>
static void gtDosageRow(const T *g, size_t n, int ploidy, int eaidx, float *out) {
    for (size_t i = 0; i < n; ++i) {
        int cnt = 0;
        bool miss = false;
        for (int k = 0; k < ploidy; ++k) {
            const int32_t a = (int32_t)g[i * (size_t)ploidy + (size_t)k];
            if (a < 0) continue;  // vector-end pad (a sample of lower ploidy)
            if (a < 2)
                miss = true;  // allele value -1
            else
                cnt += ((a >> 1) - 1) == eaidx;
        }
        out[i] = miss ? std::nanf("") : (float)cnt;
    }
}
void decodeGtDosage(const void *gts, int elem_bytes, size_t n, int ploidy, int eaidx, float *out) {
    switch (elem_bytes) {
    case 1: gtDosageRow((const int8_t *)gts, n, ploidy, eaidx, out); break;
    case 2: gtDosageRow((const int16_t *)gts, n, ploidy, eaidx, out); break;
    case 4: gtDosageRow((const int32_t *)gts, n, ploidy, eaidx, out); break;
    default: throw std::runtime_error("decodeGtDosage: FORMAT/GT elements of " + std::to_string(elem_bytes) + " bytes");
    }
}
template <class T>
static void plDosageRow(const T *p, size_t n, int n_alleles, int eaidx, const double *lik, float *out) {
    const int G = n_alleles * (n_alleles + 1) / 2;
    for (size_t i = 0; i < n; ++i, p += G) {
        double num = 0.0, den = 0.0;
        int32_t lo = INT32_MAX, hi = INT32_MIN;
        int j = 0, k = 0;  // genotype g = (j, k), j <= k
        for (int g = 0; g < G; ++g) {
            const int32_t v = (int32_t)p[g];
            lo = std::min(lo, v);
            hi = std::max(hi, v);
            const double w = lik[v < 0 ? 0 : (v > 255 ? 255 : v)];
            const int cnt = (j == eaidx) + (k == eaidx);
            num = num + (double)cnt * w;
            den = den + w;
            if (j == k) {
                j = 0;
                ++k;
            } else {
                ++j;
            }
        }
        out[i] = (lo < 0 || lo == hi) ? std::nanf("") : (float)(num / den);
    }
}
void decodePlDosage(const void *pl, int elem_bytes, size_t n, int n_alleles, int eaidx, float *out) {
    if (n_alleles < 2 || n_alleles > 8 || eaidx < 0 || eaidx >= n_alleles)
        throw std::runtime_error("decodePlDosage: " + std::to_string(n_alleles) + " alleles, effect allele " + std::to_string(eaidx));
    static const std::vector<double> lik = [] {  // the table libnps built (and uploads): nps_pl_likelihoods
        std::vector<double> t(256);
        npsCheck(nps_pl_likelihoods(t.data()), "nps_pl_likelihoods");
        return t;
    }();
    switch (elem_bytes) {
    case 1: plDosageRow((const int8_t *)pl, n, n_alleles, eaidx, lik.data(), out); break;
    case 2: plDosageRow((const int16_t *)pl, n, n_alleles, eaidx, lik.data(), out); break;
    case 4: plDosageRow((const int32_t *)pl, n, n_alleles, eaidx, lik.data(), out); break;
    default: throw std::runtime_error("decodePlDosage: FORMAT/PL elements of " + std::to_string(elem_bytes) + " bytes");
    }
}
void decodeCodeDosage(const uint8_t *codes, size_t n, int code_map, float *out) {
    // .bed: 0 = hom A1, 1 = missing, 2 = het, 3 = hom A2; .pgen: the number of ALT alleles, 3 = missing
    static const float nanv = std::nanf("");
    const float table[4][4] = {{0.f, nanv, 1.f, 2.f},   // NPS_MAP_BED_A2
                               {2.f, nanv, 1.f, 0.f},   // NPS_MAP_BED_A1
                               {0.f, 1.f, 2.f, nanv},   // NPS_MAP_PGEN_ALT
                               {2.f, 1.f, 0.f, nanv}};  // NPS_MAP_PGEN_REF
    if (code_map < 0 || code_map > 3) throw std::runtime_error("decodeCodeDosage: bad code map");
    for (size_t i = 0; i < n; ++i) out[i] = table[code_map][(codes[i >> 2] >> ((i & 3) * 2)) & 3u];
}

// ------------------------------------------------------------------------------------------
// computePolygenicScores  nim:592-649
void computePolygenicScores(std::vector<double> &scores, const ScoreFile &scoreFile,
                            const VCF &genotypeVcf, bool restrictToCoveredRgns,
                            const GenomeIntervals &coveredIvals, ImputeMethodLocus imputeMethodLocus,
                            ImputeMethodMissing imputeMethodMissing,
                            ImputeMethodSample imputeMethodSample, double maxMissingRate,
                            double afMismatchPthresh, int64_t minGtForInternalImput,
                            bool ignoreFilterField, Log &log, int device, uint64_t *nloci_out, double *d_scores_out) {
    const int64_t nsamples = genotypeVcf.n_samples();
    warmupJoin();
    const nps_params p =
        makeParams(imputeMethodLocus, imputeMethodMissing, imputeMethodSample, maxMissingRate, minGtForInternalImput);
    const Handle<nps_ctx> owner =
        created<nps_ctx>("nps_create", [&](nps_ctx **o) { return nps_create(o, device, (uint64_t)nsamples, &p); });
    nps_ctx *const ctx = owner.get();

    struct Pushed {
        const ScoreEntry *e;
        int how;  // 0 = genotyped on the device, else nps_row_kind
        std::string filter;       // FILTER of the record (for the warning text)
        std::string pre_warning;  // emitted before the device result is known (coverage contig)
    };
    std::vector<Pushed> pushed;
    pushed.reserve(scoreFile.entries.size());
    // Score rows are pushed in file order, a streaming source's one window (streamingWindow) at a time.
    const std::vector<ScoreEntry> &entries = scoreFile.entries;
    const size_t window = genotypeVcf.streaming ? streamingWindow(nsamples) : entries.size();
    std::vector<Variant> fetched;
    std::vector<float> ds_tmp;
    RecordIndex index;
    if (!genotypeVcf.streaming) index.build(genotypeVcf.records);
    for (size_t w0 = 0; w0 < entries.size(); w0 += window) {
        const size_t w1 = std::min(entries.size(), w0 + window);
        if (genotypeVcf.streaming) {
            fetched = genotypeVcf.fetch(entries.data() + w0, w1 - w0);
            index.build(fetched);
        }
        Tick tick_push(timings().push);  // (locating the records is in here too: a hash lookup per row)
        for (size_t j = w0; j < w1; ++j) {
            const ScoreEntry &e = entries[j];
            RowClass c = classifyRow(e, restrictToCoveredRgns, coveredIvals, index, ignoreFilterField);
            const Variant *v = c.v;
            const int rie = c.ref_is_effect, eaidx = c.eaidx;
            if (c.kind)  // nim:526-558: a constant row, no genotypes
                npsCheck(nps_push_locus(ctx, c.kind, rie, e.beta, e.eaf), "nps_push_locus");
            else if (v->has_pl)  // FORMAT/PL row (build-defined, NIMPRESS_FORMAT=PL): the effect allele's expected count,
                                 // decoded on the device; statistics and warnings as for a FORMAT/DS row
                npsCheck(nps_push_pl(ctx, v->pl_raw.data(), v->pl_bytes, 1 + (int)v->alt.size(), eaidx, rie, e.beta, e.eaf),
                         "nps_push_pl");
            else if (v->has_ds)  // FORMAT/DS row (build-defined; the seam of nim:381-391 for float dosages)
                npsCheck(nps_push_ds(ctx, v->dsRow(eaidx, (size_t)nsamples, ds_tmp), rie, e.beta, e.eaf),
                         "nps_push_ds");
            else if (v->is_bed || v->is_pgen)  // the .bed / fixed-width .pgen bytes as they stand in the file: recoded
                                               // on the device by the row's code map
                npsCheck(nps_push_bed(ctx, v->gt_raw.data(), c.code_map, rie, e.beta, e.eaf), "nps_push_bed");
            else if (v->gt_bytes == 4 && v->gt_raw.empty())
                npsCheck(nps_push_gt(ctx, v->gts.data(), v->ploidy, eaidx, rie, e.beta, e.eaf),
                         "nps_push_gt");
            else  // the BCF record's own int8 / int16 vector: widened on the device
                npsCheck(nps_push_gt_raw(ctx, v->gtData(), v->gt_bytes, v->ploidy, eaidx, rie,
                                         e.beta, e.eaf),
                         "nps_push_gt_raw");
            pushed.push_back(Pushed{&e, c.kind, std::move(c.filter), std::move(c.pre_warning)});
        }
    }
    // per-row results back, in order: emit the reference's warnings
    std::vector<nps_locus_stat> stats(pushed.size());
    size_t got = 0;
    npsCheck(nps_flush(ctx, stats.data(), stats.size(), &got), "nps_flush");
    if (got != pushed.size()) throw std::runtime_error("nps_flush returned too few rows");
    for (size_t j = 0; j < pushed.size(); ++j)
        writeRowWarnings(log, *pushed[j].e, pushed[j].how, pushed[j].filter, pushed[j].pre_warning, nsamples,
                         stats[j].nmissing, stats[j].neffect, stats[j].reason == NPS_REASON_MAXMIS, afMismatchPthresh);
    scores.assign((size_t)nsamples, 0.0);
    uint64_t nloci = 0;
    {
        Tick tick(timings().kernels);
        if (d_scores_out)  // the scores stay on the device (a multi-GPU gather reads them there)
            npsCheck(nps_finish_device(ctx, scoreFile.offset, d_scores_out, &nloci), "nps_finish_device");
        else
            npsCheck(nps_finish(ctx, scoreFile.offset, scores.data(), &nloci), "nps_finish");
    }
    if (d_scores_out) scores.clear();
    if (nloci_out) *nloci_out = nloci;
}

void computePolygenicScoresMulti(std::vector<std::vector<double>> &scores, const std::vector<const ScoreFile *> &scoreFiles,
                                 const VCF &genotypeVcf, bool restrictToCoveredRgns, const GenomeIntervals &coveredIvals,
                                 ImputeMethodLocus imputeMethodLocus, ImputeMethodMissing imputeMethodMissing,
                                 ImputeMethodSample imputeMethodSample, double maxMissingRate, double afMismatchPthresh,
                                 int64_t minGtForInternalImput, bool ignoreFilterField, std::vector<Log> &logs, int device,
                                 std::vector<uint64_t> *nloci_out, int shard, int n_shards, bool partial, double *d_out,
                                 bool acceptDs) {
    if (n_shards < 1 || shard < 0 || shard >= n_shards) throw std::runtime_error("computePolygenicScoresMulti: bad shard");
    warmupJoin();
    const size_t S = scoreFiles.size();
    const int64_t nsamples = genotypeVcf.n_samples();
    scores.assign(S, std::vector<double>());
    logs.assign(S, Log());
    for (Log &l : logs) l.echo = false;
    if (nloci_out) nloci_out->assign(S, 0);
    if (S == 0) return;
    const nps_params p =
        makeParams(imputeMethodLocus, imputeMethodMissing, imputeMethodSample, maxMissingRate, minGtForInternalImput);

    // ---- the union of the files' score rows: one position (= cohort row) per distinct (contig, pos, ref, ea)
    struct Position {
        ScoreEntry e;   // beta / eaf of the first file that lists it (only the locus is used)
        int how = 0;    // 0 = genotyped row, else nps_row_kind (the same for every file that lists the row)
        std::string filter, pre_warning;
    };
    std::vector<Position> pos;
    std::map<std::string, size_t> where;
    std::vector<std::vector<size_t>> rows_of(S);  // per file, in file order: the position of each score row
    for (size_t s = 0; s < S; ++s)
        for (const ScoreEntry &e : scoreFiles[s]->entries) {
            const std::string key = e.contig + "\t" + std::to_string(e.pos) + "\t" + e.refseq + "\t" + e.easeq;
            auto it = where.find(key);
            if (it == where.end()) {
                it = where.emplace(key, pos.size()).first;
                Position q;
                q.e = e;
                pos.push_back(q);
            }
            rows_of[s].push_back(it->second);
        }
    // this call's block of the union's rows (all of them unless the rows are sharded over several GPUs): cohort row
    // j - A for position j in [A, B); a file's rows outside the block are simply not part of this call's definitions
    const size_t A = pos.size() * (size_t)shard / (size_t)n_shards, B = pos.size() * ((size_t)shard + 1) / (size_t)n_shards;
    const size_t U = B - A;

    // ---- locate every position once and decode its record into the resident cohort (nim:526-561): a 2-bit cohort,
    // or -- acceptDs, from the first FORMAT/DS position on: the fill starts again -- a float32 dosage cohort
    std::vector<ScoreEntry> uent(U);
    for (size_t j = 0; j < U; ++j) uent[j] = pos[A + j].e;
    std::vector<Variant> fetched;
    RecordIndex index;
    if (!genotypeVcf.streaming) index.build(genotypeVcf.records);
    Handle<nps_cohort> gt2, dsc;
    std::vector<unsigned char> from_gt(U, 0);  // dosage cohort: the row holds effect allele counts decoded from GT
    bool as_ds = false;
    for (;;) {
        Handle<nps_cohort> &filled = as_ds ? dsc : gt2;
        filled = created<nps_cohort>("nps_cohort_create", [&](nps_cohort **o) {
            return nps_cohort_create(o, device, (uint64_t)nsamples, (uint64_t)U, as_ds ? NPS_FMT_DS32 : NPS_FMT_GT2);
        });
        // (dosage rows go up a window at a time: at most 256 MiB of them on the host)
        const size_t ds_rows = std::max<size_t>((256u << 20) / ((size_t)std::max<int64_t>(nsamples, 1) * 4), 1);
        const size_t window = genotypeVcf.streaming ? streamingWindow(nsamples) : (as_ds ? std::min(std::max<size_t>(U, 1), ds_rows) : U);
        std::vector<float> rows, ds_tmp;
        bool again = false;
        for (size_t w0 = 0; w0 < U && !again; w0 += window) {
            const size_t w1 = std::min(U, w0 + window);
            if (genotypeVcf.streaming) {
                fetched = genotypeVcf.fetch(uent.data() + w0, w1 - w0);
                index.build(fetched);
            }
            if (as_ds) rows.assign((w1 - w0) * (size_t)nsamples, 0.0f);
            for (size_t j = w0; j < w1; ++j) {  // (cohort row j = position A + j)
                Position &q = pos[A + j];
                RowClass c = classifyRow(q.e, restrictToCoveredRgns, coveredIvals, index, ignoreFilterField);
                const Variant *v = c.v;
                q.how = c.kind;
                q.filter = std::move(c.filter);
                q.pre_warning = std::move(c.pre_warning);
                if (c.kind) continue;
                Tick tick(timings().push);
                if (as_ds) {
                    float *row = rows.data() + (j - w0) * (size_t)nsamples;
                    if (v->has_pl) {  // the effect allele's expected count: the row counts the effect allele, like a GT row
                        from_gt[j] = 1;
                        decodePlDosage(v->pl_raw.data(), v->pl_bytes, (size_t)nsamples, 1 + (int)v->alt.size(), c.eaidx, row);
                    } else if (v->has_ds) {
                        memcpy(row, v->dsRow(c.eaidx, (size_t)nsamples, ds_tmp), sizeof(float) * (size_t)nsamples);
                    } else {
                        from_gt[j] = 1;
                        if (v->is_bed || v->is_pgen)
                            decodeCodeDosage(v->gt_raw.data(), (size_t)nsamples, c.code_map, row);
                        else
                            decodeGtDosage(v->gtData(), v->gt_raw.empty() ? 4 : v->gt_bytes, (size_t)nsamples, v->ploidy, c.eaidx, row);
                    }
                    continue;
                }
                if (v->has_ds || v->has_pl) {  // (a FORMAT/PL record is a dosage row too)
                    if (!acceptDs)
                        throw std::runtime_error(std::string(v->has_pl ? "FORMAT/PL" : "FORMAT/DS") +
                                                 " records are not covered by the one-pass multi-score path");
                    again = true;  // the block holds dosages: fill a float32 cohort from its first row on
                    break;
                }
                if (v->is_bed || v->is_pgen)
                    npsCheck(nps_cohort_push_bed(gt2.get(), j, v->gt_raw.data(), c.code_map), "nps_cohort_push_bed");
                else
                    npsCheck(nps_cohort_push_gt_raw(gt2.get(), j, v->gtData(), v->gt_raw.empty() ? 4 : v->gt_bytes, v->ploidy,
                                                    c.eaidx),
                             "nps_cohort_push_gt_raw");
            }
            if (as_ds && !again && nsamples > 0) {
                Tick tick(timings().push);
                npsCheck(nps_cohort_upload(dsc.get(), w0, w1 - w0, rows.data(), sizeof(float) * (size_t)nsamples), "nps_cohort_upload");
            }
        }
        if (!again) break;
        as_ds = true;
        gt2.reset();
    }
    fetched.clear();
    double t_kernels0 = nowSeconds();
    Handle<nps_cohort> gt2m;
    std::vector<uint64_t> nmiss(U, 0);
    std::vector<double> neff(U, 0.0);  // effect alleles of the genotyped samples: a count, or a dosage sum
    if (!as_ds) {
        gt2m = created<nps_cohort>("nps_cohort_create", [&](nps_cohort **o) {
            return nps_cohort_create(o, device, (uint64_t)nsamples, (uint64_t)U, NPS_FMT_GT2M);
        });
        npsCheck(nps_cohort_convert(gt2m.get(), gt2.get()), "nps_cohort_convert");
        gt2.reset();
        std::vector<uint64_t> counts(U, 0);
        if (U) npsCheck(nps_cohort_row_tallies(gt2m.get(), 0, U, nmiss.data(), counts.data()), "nps_cohort_row_tallies");
        for (size_t j = 0; j < U; ++j) neff[j] = (double)counts[j];
    }
    const nps_cohort *const cohort = as_ds ? dsc.get() : gt2m.get();

    // ---- the definitions, NPS_MULTI_MAX_SCORES files at a time
    for (size_t s0 = 0; s0 < S; s0 += NPS_MULTI_MAX_SCORES) {
        const size_t ns = std::min<size_t>(NPS_MULTI_MAX_SCORES, S - s0);
        std::vector<nps_row_desc> descs(ns * U);
        for (size_t k = 0; k < ns * U; ++k) {
            descs[k].beta = 0.0;
            descs[k].eaf = 0.0;
            descs[k].kind = NPS_ROW_NOT_IN_SCORE;
            descs[k].ref_is_effect = 0;
        }
        for (size_t s = 0; s < ns; ++s) {
            const ScoreFile &sf = *scoreFiles[s0 + s];
            for (size_t r = 0; r < sf.entries.size(); ++r) {
                if (rows_of[s0 + s][r] < A || rows_of[s0 + s][r] >= B) continue;
                const size_t j = rows_of[s0 + s][r] - A;
                nps_row_desc &d = descs[s * U + j];
                if (d.kind != NPS_ROW_NOT_IN_SCORE)
                    throw std::runtime_error("a score file lists the same locus and alleles twice: not covered by "
                                             "the one-pass multi-score path");
                d.beta = sf.entries[r].beta;
                d.eaf = sf.entries[r].eaf;
                d.kind = pos[A + j].how ? pos[A + j].how : NPS_ROW_PRESENT;
                d.ref_is_effect = (sf.entries[r].refseq == sf.entries[r].easeq ? 1 : 0) | (from_gt[j] ? NPS_RIE_COUNTS_EFFECT : 0);
            }
        }
        // (released at the end of each round in reverse order: the scorer before its definitions)
        const Handle<nps_multidef> mdef = created<nps_multidef>("nps_multidef_create", [&](nps_multidef **o) {
            return nps_multidef_create(o, device, descs.data(), (int)ns, (uint64_t)U);
        });
        const Handle<nps_multi> msc = created<nps_multi>(
            "nps_multi_create", [&](nps_multi **o) { return nps_multi_create(o, device, (uint64_t)nsamples, &p, (int)ns); });
        if (U) npsCheck(nps_score_cohort_multi(msc.get(), cohort, 0, mdef.get()), "nps_score_cohort_multi");
        if (U && as_ds && s0 == 0) {
            // the rows' tallies for the warnings: the row's, whichever batch of files lists it (every pass counts all rows);
            // the flipped sum where the row's dosage is 2 - DS
            std::vector<double> sum(U), flipped(U);
            npsCheck(nps_multi_row_tallies(msc.get(), 0, U, nmiss.data(), sum.data(), flipped.data()), "nps_multi_row_tallies");
            for (size_t j = 0; j < U; ++j)
                neff[j] = !from_gt[j] && pos[A + j].e.refseq == pos[A + j].e.easeq ? flipped[j] : sum[j];
        }
        std::vector<double> offs(ns), flat(ns * (size_t)std::max<int64_t>(nsamples, 1));
        std::vector<uint64_t> nl(ns, 0);
        for (size_t s = 0; s < ns; ++s) offs[s] = scoreFiles[s0 + s]->offset;
        double *d_dst = d_out ? d_out + s0 * (size_t)nsamples : nullptr;  // [S][nsamples] on the device
        if (d_dst && partial)
            npsCheck(nps_multi_partial_device(msc.get(), d_dst, nl.data()), "nps_multi_partial_device");
        else if (d_dst)
            npsCheck(nps_multi_finish_device(msc.get(), offs.data(), d_dst, nl.data()), "nps_multi_finish_device");
        else if (partial)
            npsCheck(nps_multi_partial(msc.get(), flat.data(), nl.data()), "nps_multi_partial");
        else
            npsCheck(nps_multi_finish(msc.get(), offs.data(), flat.data(), nl.data()), "nps_multi_finish");
        for (size_t s = 0; s < ns; ++s) {
            if (!d_dst)
                scores[s0 + s].assign(flat.begin() + (ptrdiff_t)(s * (size_t)nsamples),
                                      flat.begin() + (ptrdiff_t)((s + 1) * (size_t)nsamples));
            if (nloci_out) (*nloci_out)[s0 + s] = nl[s];
        }
    }

    timings().kernels += nowSeconds() - t_kernels0;
    // ---- the reference's warnings, per file in its own row order (nim:527-579), from the rows' tallies
    Tick tick_warn(timings().warnings);
    for (size_t s = 0; s < S; ++s) {
        const ScoreFile &sf = *scoreFiles[s];
        for (size_t r = 0; r < sf.entries.size(); ++r) {
            if (rows_of[s][r] < A || rows_of[s][r] >= B) continue;
            const Position &q = pos[rows_of[s][r]];
            const size_t j = rows_of[s][r] - A;
            const bool over_maxmis = (double)nmiss[j] / (double)nsamples > maxMissingRate;  // nim:565
            writeRowWarnings(logs[s], sf.entries[r], q.how, q.filter, q.pre_warning, nsamples, nmiss[j], neff[j], over_maxmis,
                             afMismatchPthresh);
        }
    }
}

}  // namespace nimpress
