// nps_engine.hip -- implementation of the C-ABI declared in include/nps.h.
//
// Host-side orchestration only: staging, batching, launches, bookkeeping of per-row stats.  All
// per-sample arithmetic happens in nps_kernels.hip (and nps_fused.hip).  There is no CPU compute
// path here: if HIP is unusable every entry point that would compute returns NPS_E_NODEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <new>
#include <string>
#include <mutex>
#include <vector>

#include "nps_kernels.h"
#include "nps_own.h"
#include "nps_subset_mask.h"

using namespace nps;

extern "C" int64_t nps_live_resources(void) { return live_resources.load(); }

// ------------------------------------------------------------------------------------------
// errors
static thread_local std::string g_last_error;

static int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return fail(_e == hipErrorOutOfMemory ? NPS_E_NOMEM : NPS_E_HIP, "%s failed: %s",  \
                        #expr, hipGetErrorString(_e));                                         \
    } while (0)

// ------------------------------------------------------------------------------------------
enum ProfClass { P_DECODE = 0, P_TALLY, P_PARAMS, P_ACCUM, P_FUSED, P_REDUCE, P_COUNT };

struct ProfSpan {
    Event a, b;
    int cls;
};

struct nps_cohort {
    // nps_cohort_push_*: rows decoded on the device straight into the cohort (a pinned ring the decode kernel reads
    // over PCIe, on a stream of the cohort's own); every call that reads the cohort waits for it (cohort_quiesce)
    Stream push_stream;  // (first: destroyed last)
    int device = 0;
    int format = NPS_FMT_GT2;
    uint64_t n_samples = 0, n_rows = 0;
    uint64_t stride_bytes = 0;  // per row (GT2: rows are interleaved in groups of 4, a group is 4*stride_bytes)
    DevBuf<unsigned char> d_data;
    // nps_cohort_optimize (GT2): the rows are in the parity layout (nps_kernels.h: the high-bit plane of
    // slot 0 of every group holds the XOR of the four rows' planes)
    bool optimized = false;
    // NPS_FMT_GT2M: whole-row tallies (nmissing << 32 | neffect) produced by whatever packed the rows
    DevBuf<unsigned long long> d_row_tally;
    // NPS_FMT_GT2X: the whole-row tallies (nmissing << 28 | neffect, the tally word of the strip kernel without its arrival
    // count), one per row of every superblock, allocated (zeroed) on first need.  Counted where the rows are written
    // (upload, upload_bed, convert: the fill kernels), by nps_cohort_keep_tallies, or kept from a scoring pass.
    DevBuf<unsigned long long> d_mx_row_tally;
    // Which superblocks' words are complete: one bit per superblock (mx_sb_valid) and the number of bits set.  Contexts on
    // several threads may score one cohort: every WRITER of d_mx_row_tally, of the bitmap and of mx_tally_asked holds
    // tally_mutex and sets a bit (release) only AFTER the superblock's words are in device memory; readers load with
    // acquire and never see a superblock valid whose words are still on their way.
    std::unique_ptr<std::atomic<uint64_t>[]> mx_sb_valid;
    std::atomic<uint64_t> mx_sb_valid_count{0};
    // "asked for": nps_cohort_keep_tallies, or a pass that kept them (nps_cohort_expect_passes / the nine-tenths rule) --
    // NPS_MODE_AUTO then scores valid runs with the tallies given at ANY size; cleared by every rewrite
    std::atomic<bool> mx_tally_asked{false};
    std::mutex tally_mutex;  // NPS_MODE_AUTO may count them lazily from whichever context scores the cohort first
    std::atomic<uint32_t> expect_passes{0};  // nps_cohort_expect_passes: how often the caller will score this cohort (0: not said)
    StagingRing push{2};  // the ring of nps_cohort_push_* (grows to the widest row pushed)
    DevBuf<unsigned long long> d_push_tally;  // scratch word for the decode kernel's tally (a GT2 cohort keeps none)
    // NPS_FMT_DS32: rows that hold a value outside [0, 2] (checked when rows are uploaded; the generator clips): while
    // there is one, the cohort is scored by the two-pass kernels (the single-read kernel's fixed-point tallies need the range)
    std::vector<unsigned char> ds_row_bad;
    uint64_t ds_bad_rows = 0;

    ~nps_cohort() {  // nothing on the device may still read or write what the members release
        (void)hipSetDevice(device);
        (void)hipDeviceSynchronize();
    }
};

// ---- NPS_FMT_GT2X: which superblocks carry their tally words ------------------------------------------------------
static bool mx_tallies_valid(const nps_cohort *c, uint64_t sb0, uint64_t n_sb) {
    if (!c->mx_sb_valid) return n_sb == 0;
    if (n_sb == gt2x_superblocks(c->n_rows)) return c->mx_sb_valid_count.load(std::memory_order_acquire) == n_sb;
    for (uint64_t sb = sb0; sb < sb0 + n_sb; ++sb)
        if (!((c->mx_sb_valid[sb >> 6].load(std::memory_order_acquire) >> (sb & 63)) & 1ull)) return false;
    return true;
}
static bool mx_tallies_all_valid(const nps_cohort *c) { return mx_tallies_valid(c, 0, gt2x_superblocks(c->n_rows)); }
// tally_mutex held.  valid = true only once the words of these superblocks ARE in device memory.
static void mx_tallies_mark(nps_cohort *c, uint64_t sb0, uint64_t n_sb, bool valid) {
    if (!c->mx_sb_valid) return;
    uint64_t count = c->mx_sb_valid_count.load(std::memory_order_relaxed);
    for (uint64_t sb = sb0; sb < sb0 + n_sb; ++sb) {
        const uint64_t bit = 1ull << (sb & 63), w = c->mx_sb_valid[sb >> 6].load(std::memory_order_relaxed);
        if (((w & bit) != 0) == valid) continue;
        c->mx_sb_valid[sb >> 6].store(valid ? w | bit : w & ~bit, std::memory_order_release);
        count += valid ? 1 : (uint64_t)-1;
    }
    c->mx_sb_valid_count.store(count, std::memory_order_release);
}
// tally_mutex held, the cohort's device current
static hipError_t mx_tallies_alloc(nps_cohort *c) {
    if (c->d_mx_row_tally.get()) return hipSuccess;
    const uint64_t words = std::max<uint64_t>(gt2x_superblocks(c->n_rows) * 128, 1);
    hipError_t e = c->d_mx_row_tally.alloc(words);
    if (e == hipSuccess) e = hipMemset(c->d_mx_row_tally.get(), 0, sizeof(unsigned long long) * words);
    if (e != hipSuccess) c->d_mx_row_tally.reset();
    return e;
}
// a call that rewrites rows [row0, row0 + nrows) of a strip cohort: their superblocks carry nothing until the writer says so
static void mx_tallies_rewrite(nps_cohort *c, uint64_t row0, uint64_t nrows) {
    if (c->format != NPS_FMT_GT2X || nrows == 0) return;
    std::lock_guard<std::mutex> lk(c->tally_mutex);
    c->mx_tally_asked.store(false, std::memory_order_relaxed);
    mx_tallies_mark(c, row0 >> 7, ((row0 + nrows + 127) >> 7) - (row0 >> 7), false);
}

static int mx_keep_tallies_locked(nps_cohort *c);

static int cohort_quiesce(const nps_cohort *c) {
    if (c && c->push_stream.get()) HIP_TRY(hipStreamSynchronize(c->push_stream.get()));
    return NPS_OK;
}

// A chosen subset of a cohort's samples (nps_score_cohort_def_subset): the mask of nps_subset_mask.h on the device,
// immutable after creation -- contexts on several threads may share one.
struct nps_sampleset {
    int device = 0;
    uint64_t n_samples = 0, n_kept = 0;
    DevBuf<uint32_t> d_bits;             // one bit per sample (the masked dosage tally, the gather)
    DevBuf<unsigned long long> d_unit;   // one word per unit of the strip layout (the masked strip tally)
    DevBuf<uint32_t> d_prefix;           // kept samples in front of every word of d_bits (the gather)

    ~nps_sampleset() {  // queued work may still read the mask
        (void)hipSetDevice(device);
        (void)hipDeviceSynchronize();
    }
};

struct PendingRow {
    int32_t batch_idx;  // >= 0: index into the open GT / DS batch's device stats; -1: host stat
    int32_t is_ds;      // which open batch batch_idx refers to
    nps_locus_stat host;
};

// the rows pushed since the last run_batch, GT or FORMAT/DS: what the host knows of them and, after the run, their statistics
struct OpenBatch {
    uint32_t cap = 0, rows = 0;
    nps_row_desc *h_desc = nullptr;     // pinned [cap]
    nps_locus_stat *h_stats = nullptr;  // pinned [cap]
};

struct MxOpRow {  // nps_mxg.hip (tallies given): the weight operands of one row
    unsigned char bytes[48];
};

struct nps_ctx {
    Stream stream;  // (first: destroyed last)
    int device = 0;
    uint64_t n = 0;         // samples
    uint64_t n_words = 0;   // ceil(n/16)
    uint64_t stride_words = 0;
    nps_params params{};

    // streaming batch
    OpenBatch gt;
    DevBuf<uint32_t> d_codes;               // [gt.cap/4 groups][stride_words][4] (interleaved)
    DevBuf<unsigned long long> d_tally;     // [gt.cap]
    DevBuf<nps_row_desc> d_desc;            // [gt.cap]
    DevBuf<double> d_lut;                   // [gt.cap][4]
    DevBuf<nps_locus_stat> d_stats;         // [gt.cap]
    PinnedBuf h_arena;      // ONE pinned allocation holding h_result, gt.h_desc and gt.h_stats
    StagingRing raw{8};     // diploid GT, packed and .bed rows in flight between the caller's buffer and the device

    // FORMAT/DS streaming batch (ensure_ds: allocated on the first row that needs it)
    OpenBatch ds;
    uint64_t ds_stride_f = 0;
    DevBuf<float> d_ds;                  // [ds.cap][ds_stride_f]
    DevBuf<nps_row_desc> d_ds_desc;      // [ds.cap]
    DevBuf<DsTally> d_ds_tally;
    DevBuf<DsRowP> d_ds_rowp;
    DevBuf<nps_locus_stat> d_ds_stats;
    PinnedBuf h_ds_arena;                // pinned: ds.h_desc, ds.h_stats
    StagingRing ds_raw{2};               // rows of nps_push_ds
    // resident DS runs (grown on demand)
    DevBuf<DsTally> d_rds_tally;
    DevBuf<DsRowP> d_rds_rowp;

    StagingRing poly{2};  // raw GT records of ploidy > 2, read by the decode kernel (grows to the widest record pushed)
    StagingRing pl{4};    // FORMAT/PL vectors of nps_push_pl, read by decode_pl_kernel (grows to the widest record pushed)

    // accumulators
    AccumGeom geom{};         // streaming geometry (groups_per_chunk for a full batch)
    uint32_t n_chunks = 1;
    DevBuf<double> d_part;  // [n_chunks][part_chunk_stride]
    // which chunks of d_part hold data: 0 = none yet (nothing has been zeroed either: the first
    // writer overwrites), 1 = chunk 0 only (fused epilogues), n_chunks = all (two-pass kernels)
    uint32_t chunks_used = 0;
    DevBuf<double> d_scores;
    DevBuf<double> d_subset_scores;          // nps_finish_subset: the kept samples' scores on their way to the host
    DevBuf<unsigned long long> d_nloci;      // [0] used rows counted on the device, [1] sticky status bits
    unsigned long long *h_result = nullptr;  // pinned copy of that block
    bool broken = false;                     // a launch sequence failed half-way: nps_reset first
    double const_sum = 0.0;   // contributions of rows without genotype data (host decided)
    uint64_t host_nloci = 0;

    // resident runs (nps_score_cohort*): per-row buffers, grown on demand
    DevBuf<unsigned long long> d_rtally;    // [rows] (a pair per row for the single-read DS kernel)
    DevBuf<double> d_rlut;                  // [rows][4]
    DevBuf<nps_locus_stat> d_rstats;        // [rows]
    DevBuf<double> d_part_fused;            // [Q][team stride] partial scores of the fused kernel
    DevBuf<unsigned int> d_timeout;         // bounded-wait flag of the fused kernels (cleared by fold_kernel)
    DevBuf<float> d_mx_cpart;               // NPS_FMT_GT2X runs: digit sums handed from fused_mx_kernel to mx_fold_kernel
    DevBuf<double> d_mx_const;              // ... and the locus constants of rows over --maxmis: [8 scratch][2 Q slots], zero between passes
    DevBuf<unsigned long long> d_mx_tally1; // first-stage tally words (groups of 16 strips), zero between passes
    DevBuf<MxOpRow> d_mx_ops;               // nps_mxg.hip (tallies given): the weight operands of every row ...
    DevBuf<double> d_mx_cblk;               // ... and one partial sum of locus constants per superblock
    // NPS_FMT_GT2X runs of a definition with special rows (nps_scoredef::special): those rows in the row layout, scored
    // in IEEE double by the two-pass kernels, a batch at a time
    DevBuf<uint32_t> d_sp_plain;                // [batch][n_words] plain rows out of the strip layout
    DevBuf<uint32_t> d_sp_group;                // [batch / 4 groups][stride_words][4] interleaved
    DevBuf<unsigned long long> d_sp_tally;      // [batch]
    DevBuf<double> d_sp_lut;                    // [batch][4]
    bool rtally_clean = false;              // d_rtally is all zero (allocation, or the last fused epilogue)
    // shape -> persistent-grid plan of the last resident run (occupancy queries are slow)
    bool plan_valid = false;
    int plan_fmt = -1;
    uint64_t plan_m = 0;
    FusedPlan plan_cache{};
    bool res_pending = false;               // stats of the last resident run still on the device
    uint64_t res_m = 0;
    std::vector<int64_t> res_index;
    std::vector<nps_locus_stat> res_host_stats;

    // stats in push order
    std::vector<PendingRow> pending;        // rows of the open batch (+ no-data rows since)
    std::vector<nps_locus_stat> ready;      // completed, not yet returned by nps_flush
    size_t ready_cursor = 0;

    // profiling
    bool profiling = false;
    std::vector<ProfSpan> spans;
    nps_profile prof{};

    ~nps_ctx() {  // queued work may still use what the members release
        (void)hipSetDevice(device);
        if (stream.get()) (void)hipStreamSynchronize(stream.get());
    }
};

static DevParams dev_params(const nps_params &p) {
    DevParams d;
    d.imp_locus = p.imp_locus;
    d.imp_missing = p.imp_missing;
    d.imp_sample = p.imp_sample;
    d.max_missing_rate = p.max_missing_rate;
    d.min_cs = (double)p.min_cs;
    return d;
}

static int check_params(const nps_params *p) {
    if (!p) return fail(NPS_E_INVAL, "params is NULL");
    if (p->imp_locus < 0 || p->imp_locus > NPS_LOCUS_IGNORE)
        return fail(NPS_E_INVAL, "imp_locus %d out of range", p->imp_locus);
    if (p->imp_missing < 0 || p->imp_missing > NPS_MISSING_IGNORE)
        return fail(NPS_E_INVAL, "imp_missing %d out of range", p->imp_missing);
    if (p->imp_sample < 0 || p->imp_sample > NPS_SAMPLE_INT_FAIL)
        return fail(NPS_E_INVAL, "imp_sample %d out of range", p->imp_sample);
    return NPS_OK;
}

// profiling helpers -------------------------------------------------------------------------
struct ProfScope {
    nps_ctx *c;
    int cls;
    Event a, b;
    ProfScope(nps_ctx *ctx, int k) : c(ctx), cls(k) {
        if (c->profiling && a.create(hipEventDefault) == hipSuccess && b.create(hipEventDefault) == hipSuccess)
            (void)hipEventRecord(a.get(), c->stream.get());
    }
    ~ProfScope() {
        if (b.get()) {
            (void)hipEventRecord(b.get(), c->stream.get());
            c->spans.push_back({std::move(a), std::move(b), cls});
        }
    }
};

static void resolve_spans(nps_ctx *c) {
    for (auto &s : c->spans) {
        float ms = 0.f;
        (void)hipEventSynchronize(s.b.get());
        (void)hipEventElapsedTime(&ms, s.a.get(), s.b.get());
        double *acc[P_COUNT] = {&c->prof.ms_decode, &c->prof.ms_tally,  &c->prof.ms_params,
                                &c->prof.ms_accumulate, &c->prof.ms_fused, &c->prof.ms_reduce};
        uint64_t *cnt[P_COUNT] = {&c->prof.n_decode, &c->prof.n_tally,  &c->prof.n_params,
                                  &c->prof.n_accumulate, &c->prof.n_fused, &c->prof.n_reduce};
        *acc[s.cls] += ms;
        *cnt[s.cls] += 1;
    }
    c->spans.clear();
}

// ------------------------------------------------------------------------------------------
extern "C" int nps_abi_version(void) { return NPS_ABI_VERSION; }
extern "C" const char *nps_last_error(void) { return g_last_error.c_str(); }

extern "C" int nps_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static int select_device(int device);
__global__ void warmup_kernel(unsigned int *p) {
    if (p) *p = 1u;
}
extern "C" int nps_warmup(int device) {
    int rc = select_device(device);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());  // the primary context
    (void)hipGetLastError();
    hipLaunchKernelGGL(warmup_kernel, dim3(1), dim3(1), 0, nullptr, (unsigned int *)nullptr);  // the code object
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return NPS_OK;
}

static int select_device(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(NPS_E_NODEVICE, "no HIP device available (%s); libnps has no CPU path",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device < 0 || device >= n)
        return fail(NPS_E_NODEVICE, "device %d out of range (have %d)", device, n);
    HIP_TRY(hipSetDevice(device));
    return NPS_OK;
}

// geometry of the partial-score buffer: sample tiles x row chunks >= ~2048 blocks
static void choose_geometry(nps_ctx *c) {
    const uint32_t tiles = (uint32_t)std::max<uint64_t>(1, (c->n_words + 255) / 256);
    uint32_t chunks = (2048 + tiles - 1) / tiles;
    chunks = std::max(1u, std::min(chunks, 64u));
    c->n_chunks = chunks;
    c->geom.n_words = (uint32_t)c->n_words;
    c->geom.n_chunks = chunks;
    c->geom.part_chunk_stride = (uint64_t)tiles * 256 * 16;
}

static int zero_state(nps_ctx *c) {
    // d_part is not touched: chunks_used = 0 makes the first writer overwrite it
    HIP_TRY(hipMemsetAsync(c->d_nloci.get(), 0, 3 * sizeof(unsigned long long), c->stream.get()));
    if (c->gt.rows)  // tallies of rows decoded into the open batch (the array is zero otherwise)
        HIP_TRY(hipMemsetAsync(c->d_tally.get(), 0, sizeof(unsigned long long) * c->gt.rows, c->stream.get()));
    c->chunks_used = 0;
    c->broken = false;
    c->const_sum = 0.0;
    c->host_nloci = 0;
    c->gt.rows = 0;
    c->ds.rows = 0;
    c->pending.clear();
    c->ready.clear();
    c->ready_cursor = 0;
    c->res_pending = false;  // unflushed stats of a resident run are dropped, never copied
    c->res_index.clear();
    c->res_host_stats.clear();
    return NPS_OK;
}

// the two-pass kernels add into every chunk of d_part: zero the chunks nothing has written yet
static int ensure_all_chunks(nps_ctx *c) {
    if (c->chunks_used < c->n_chunks) {
        HIP_TRY(hipMemsetAsync(c->d_part.get() + (uint64_t)c->chunks_used * c->geom.part_chunk_stride, 0,
                               sizeof(double) * (c->n_chunks - c->chunks_used) * c->geom.part_chunk_stride,
                               c->stream.get()));
        c->chunks_used = c->n_chunks;
    }
    return NPS_OK;
}

extern "C" int nps_create(nps_ctx **out, int device, uint64_t n_samples, const nps_params *params) {
    if (!out) return fail(NPS_E_INVAL, "out is NULL");
    *out = nullptr;
    int rc = check_params(params);
    if (rc) return rc;
    if (n_samples > 0x7fffffffull)
        return fail(NPS_E_UNSUPPORTED, "n_samples %llu exceeds 2^31-1",
                    (unsigned long long)n_samples);
    rc = select_device(device);
    if (rc) return rc;
    std::unique_ptr<nps_ctx> owner(new (std::nothrow) nps_ctx);
    nps_ctx *c = owner.get();
    if (!c) return fail(NPS_E_NOMEM, "out of host memory");
    c->device = device;
    c->n = n_samples;
    c->n_words = words_for(n_samples);
    c->stride_words = stride_words_for(n_samples);
    c->params = *params;
    choose_geometry(c);

    const uint64_t row_words = c->stride_words;
    uint64_t cap = (64ull << 20) / (row_words * 4);
    cap = std::max<uint64_t>(16, std::min<uint64_t>(cap, 4096));
    cap = cap / 16 * 16;
    c->gt.cap = (uint32_t)cap;
    c->geom.groups_per_chunk =
        std::max(1u, ((c->gt.cap / 4) + c->n_chunks - 1) / c->n_chunks);

    HIP_TRY(c->stream.create());
    HIP_TRY(c->d_codes.alloc(row_words * c->gt.cap));
    HIP_TRY(hipMemsetAsync(c->d_codes.get(), 0, row_words * 4 * c->gt.cap, c->stream.get()));
    HIP_TRY(c->d_tally.alloc(c->gt.cap));
    HIP_TRY(c->d_desc.alloc(c->gt.cap));
    {
        // One pinned arena for the result block and the batch's host arrays, carved at 4 KiB boundaries, padded to 64 KiB.
        auto up = [](size_t v) { return (v + 4095) / 4096 * 4096; };
        const size_t sz_desc = up(sizeof(nps_row_desc) * c->gt.cap);
        const size_t sz_stats = up(sizeof(nps_locus_stat) * c->gt.cap);
        const size_t total = (4096 + sz_desc + sz_stats + 65535) / 65536 * 65536;
        HIP_TRY(c->h_arena.alloc(total));
        char *p = (char *)c->h_arena.get();
        c->h_result = (unsigned long long *)p;
        c->h_result[0] = c->h_result[1] = c->h_result[2] = 0;
        p += 4096;
        c->gt.h_desc = (nps_row_desc *)p;
        p += sz_desc;
        c->gt.h_stats = (nps_locus_stat *)p;
    }
    // a slot holds the widest diploid record: two int32 per sample
    HIP_TRY(c->raw.ensure(sizeof(int32_t) * 2 * std::max<uint64_t>(c->n, 1), c->stream.get()));
    HIP_TRY(c->d_lut.alloc(4ull * c->gt.cap));
    HIP_TRY(c->d_stats.alloc(c->gt.cap));
    HIP_TRY(c->d_part.alloc(c->n_chunks * c->geom.part_chunk_stride));
    HIP_TRY(c->d_scores.alloc(std::max<uint64_t>(c->n, 1)));
    HIP_TRY(c->d_nloci.alloc(256 / sizeof(unsigned long long)));
    HIP_TRY(c->d_timeout.alloc(256 / sizeof(unsigned int)));
    HIP_TRY(hipMemsetAsync(c->d_timeout.get(), 0, 256, c->stream.get()));
    HIP_TRY(hipMemsetAsync(c->d_tally.get(), 0, sizeof(unsigned long long) * c->gt.cap, c->stream.get()));
    rc = zero_state(c);
    if (rc) return rc;
    *out = owner.release();
    return NPS_OK;
}

extern "C" void nps_destroy(nps_ctx *ctx) { delete ctx; }
extern "C" uint64_t nps_n_samples(const nps_ctx *ctx) { return ctx ? ctx->n : 0; }
extern "C" int nps_device(const nps_ctx *ctx) { return ctx ? ctx->device : -1; }

extern "C" int nps_reset(nps_ctx *c, const nps_params *params) {
    if (!c) return fail(NPS_E_INVAL, "ctx is NULL");
    if (params) {
        int rc = check_params(params);
        if (rc) return rc;
        c->params = *params;
    }
    HIP_TRY(hipSetDevice(c->device));
    // no stream synchronisation: everything below is ordered on the context's stream, and no call
    // returns with a device-to-host copy still in flight
    return zero_state(c);
}

// ------------------------------------------------------------------------------------------
// rows without genotype data are decided entirely on the host: nimpress.nim:526-558 + 417-447
static void host_locus_row(nps_ctx *c, int kind, int rie, double beta, double eaf,
                           nps_locus_stat *st) {
    const RowDecision d = no_data_row(dev_params(c->params), kind, eaf, rie != 0);
    *st = row_stat(d, 0, 0, 0.0);
    if (d.used) {
        volatile double term = d.imp * beta;  // same product as nimpress.nim:640, not contracted
        c->const_sum += term;
        c->host_nloci += 1;
    }
}

static int check_usable(nps_ctx *c) {
    if (!c) return fail(NPS_E_INVAL, "ctx is NULL");
    if (c->broken)
        return fail(NPS_E_STATE, "a previous call on this context failed half-way through its launches; "
                                 "call nps_reset before using it again");
    return NPS_OK;
}

static int materialize_resident_stats(nps_ctx *c);

// run the open batch: params -> accumulate; then collect its stats
static int run_batch(nps_ctx *c) {
    if (c->res_pending && !c->pending.empty()) {  // keep stats in push order
        int rc = materialize_resident_stats(c);
        if (rc) return rc;
    }
    if (c->gt.rows == 0 && c->ds.rows == 0) {
        // only host rows pending: move them to ready
        for (auto &p : c->pending) c->ready.push_back(p.host);
        c->pending.clear();
        return NPS_OK;
    }
    const uint32_t rows = c->gt.rows;
    if (rows) {
        const uint32_t rows_pad = (rows + 3) / 4 * 4;
        HIP_TRY(hipMemcpyAsync(c->d_desc.get(), c->gt.h_desc, sizeof(nps_row_desc) * rows,
                               hipMemcpyHostToDevice, c->stream.get()));
        {
            ProfScope ps(c, P_PARAMS);
            HIP_TRY(launch_row_params(c->stream.get(), c->d_tally.get(), c->d_desc.get(), rows, rows_pad, c->n,
                                      dev_params(c->params), c->d_lut.get(), c->d_stats.get(), c->d_nloci.get()));
        }
        if (c->n) {
            int rc = ensure_all_chunks(c);
            if (rc) return rc;
            ProfScope ps(c, P_ACCUM);
            HIP_TRY(launch_accumulate(c->stream.get(), c->d_codes.get(), c->stride_words, rows, c->d_lut.get(), c->geom,
                                      c->d_part.get()));
        }
        HIP_TRY(hipMemcpyAsync(c->gt.h_stats, c->d_stats.get(), sizeof(nps_locus_stat) * rows,
                               hipMemcpyDeviceToHost, c->stream.get()));
        HIP_TRY(hipMemsetAsync(c->d_tally.get(), 0, sizeof(unsigned long long) * rows, c->stream.get()));
    }
    const uint32_t drows = c->ds.rows;
    if (drows) {
        HIP_TRY(hipMemcpyAsync(c->d_ds_desc.get(), c->ds.h_desc, sizeof(nps_row_desc) * drows,
                               hipMemcpyHostToDevice, c->stream.get()));
        {
            ProfScope ps(c, P_TALLY);
            HIP_TRY(launch_ds_tally(c->stream.get(), c->d_ds.get(), c->ds_stride_f, c->n, c->d_ds_desc.get(), drows,
                                    nullptr, c->d_ds_tally.get()));
        }
        {
            ProfScope ps(c, P_PARAMS);
            HIP_TRY(launch_ds_params(c->stream.get(), c->d_ds_tally.get(), c->d_ds_desc.get(), drows, c->n,
                                     dev_params(c->params), c->d_ds_rowp.get(), c->d_ds_stats.get(), c->d_nloci.get()));
        }
        {
            int rc = ensure_all_chunks(c);
            if (rc) return rc;
            ProfScope ps(c, P_ACCUM);
            HIP_TRY(launch_ds_accumulate(c->stream.get(), c->d_ds.get(), c->ds_stride_f, c->n, c->d_ds_rowp.get(), drows,
                                         c->d_part.get(), c->n_chunks, c->geom.part_chunk_stride));
        }
        HIP_TRY(hipMemcpyAsync(c->ds.h_stats, c->d_ds_stats.get(), sizeof(nps_locus_stat) * drows,
                               hipMemcpyDeviceToHost, c->stream.get()));
    }
    HIP_TRY(hipStreamSynchronize(c->stream.get()));
    for (auto &p : c->pending)
        c->ready.push_back(p.batch_idx < 0 ? p.host : (p.is_ds ? c->ds : c->gt).h_stats[p.batch_idx]);
    c->pending.clear();
    c->gt.rows = 0;
    c->ds.rows = 0;
    return NPS_OK;
}

// open the next row of batch `b` (run the batches first when it is full) and fill in its descriptor; row_flags: bits of
// nps_row_desc::ref_is_effect above bit 0
static int begin_data_row(nps_ctx *c, OpenBatch &b, int ref_is_effect, int row_flags, double beta, double eaf,
                          uint32_t *slot) {
    if (b.rows == b.cap) {
        int rc = run_batch(c);
        if (rc) return rc;
    }
    *slot = b.rows;
    nps_row_desc &d = b.h_desc[*slot];
    d.beta = beta;
    d.eaf = eaf;
    d.kind = NPS_ROW_PRESENT;
    d.ref_is_effect = (ref_is_effect ? 1 : 0) | row_flags;
    return NPS_OK;
}

static void commit_data_row(nps_ctx *c, OpenBatch &b, uint32_t slot) {
    PendingRow p;
    p.batch_idx = (int32_t)slot;
    p.is_ds = &b == &c->ds;
    memset(&p.host, 0, sizeof p.host);
    c->pending.push_back(p);
    b.rows = slot + 1;
}

// One row through a staging ring.  The caller may reuse its buffer on return, so `fill` copies it into the next pinned
// slot; `queue` queues on `st` the work that reads the slot where it lies (a kernel, over PCIe: one launch per row instead
// of a DMA copy and a launch that wait for each other, ~50 us per row); the slot's event goes behind it.  No stream
// synchronisation per row; if `queue` fails no event is recorded.
template <class Fill, class Queue>
static int stage_row(StagingRing &ring, hipStream_t st, Fill fill, Queue queue) {
    void *slot = nullptr;
    HIP_TRY(ring.acquire(&slot));
    fill(slot);
    int rc = queue(slot);
    if (rc) return rc;
    HIP_TRY(ring.release(st));
    return NPS_OK;
}

// a .bed / .pgen row of n samples into a slot: ceil(n/4) bytes, zero up to the word boundary
static void stage_bed_row(void *slot, const uint8_t *bed_row, uint64_t n) {
    const size_t bytes = (size_t)((n + 3) / 4), padded = sizeof(uint32_t) * words_for(n);
    memcpy(slot, bed_row, bytes);
    memset((char *)slot + bytes, 0, padded - bytes);
}

// the typed GT vector of a record; max_ploidy: what the destination holds
static int check_raw_gt(int elem_bytes, int ploidy, int eaidx, int max_ploidy) {
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4)
        return fail(NPS_E_INVAL, "elem_bytes %d (1, 2 or 4)", elem_bytes);
    if (ploidy < 1) return fail(NPS_E_INVAL, "ploidy %d < 1", ploidy);
    if (ploidy > max_ploidy)
        return max_ploidy == 2 ? fail(NPS_E_UNSUPPORTED, "ploidy %d > 2 does not fit the 2-bit cohort", ploidy)
                               : fail(NPS_E_UNSUPPORTED, "ploidy %d > 8", ploidy);
    if (eaidx < 0) return fail(NPS_E_INVAL, "eaidx %d < 0 (nimpress.nim:380 doAssert)", eaidx);
    return NPS_OK;
}

static int ensure_ds(nps_ctx *c);

// ploidy > 2: the dosage can exceed 2, which the 2-bit codes cannot hold (nimpress is documented as
// diploid-specific, README.md:158, but its loop counts any number of alleles, nim:385-390).  The
// record is decoded on the device into a float dosage row and scored through the DS path.
static int push_gt_polyploid(nps_ctx *c, const void *gts, int elem_bytes, int ploidy, int eaidx,
                             int ref_is_effect, double beta, double eaf) {
    int rc = ensure_ds(c);
    if (rc) return rc;
    // the decoded row already counts the effect allele: flag bit 1 tells the DS kernels not to apply
    // the 2 - DS transform, bit 0 still selects the homref imputation value (nim:435-438)
    uint32_t slot;
    rc = begin_data_row(c, c->ds, ref_is_effect, 2, beta, eaf, &slot);
    if (rc) return rc;
    if (c->n) {
        const size_t bytes = (size_t)elem_bytes * (size_t)ploidy * c->n;
        HIP_TRY(c->poly.ensure(bytes, c->stream.get()));  // (rare: once or twice per context)
        rc = stage_row(c->poly, c->stream.get(), [&](void *s) { memcpy(s, gts, bytes); }, [&](void *s) -> int {
            ProfScope ps(c, P_DECODE);
            HIP_TRY(launch_decode_gt_to_ds(c->stream.get(), s, elem_bytes, c->n, ploidy, eaidx,
                                           c->d_ds.get() + (uint64_t)slot * c->ds_stride_f));
            return NPS_OK;
        });
        if (rc) return rc;
    }
    commit_data_row(c, c->ds, slot);
    return NPS_OK;
}

// the typed FORMAT/PL vector of a diploid record with n_alleles alleles (REF + ALTs)
static int check_raw_pl(int elem_bytes, int n_alleles, int eaidx) {
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4)
        return fail(NPS_E_INVAL, "elem_bytes %d (1, 2 or 4)", elem_bytes);
    if (n_alleles < 2 || n_alleles > 8) return fail(NPS_E_UNSUPPORTED, "FORMAT/PL of %d alleles (2 .. 8)", n_alleles);
    if (eaidx < 0 || eaidx >= n_alleles) return fail(NPS_E_INVAL, "eaidx %d outside the %d alleles", eaidx, n_alleles);
    return NPS_OK;
}

extern "C" int nps_pl_likelihoods(double *out256) {
    if (!out256) return fail(NPS_E_INVAL, "out256 is NULL");
    memcpy(out256, pl_likelihood_table(), 256 * sizeof(double));
    return NPS_OK;
}

// PRESENT row with FORMAT/PL (build-defined, include/nps.h): like a polyploid GT record, the vector is decoded on the
// device into a float dosage row that already counts the effect allele, and scored through the DS path
extern "C" int nps_push_pl(nps_ctx *c, const void *pl, int elem_bytes, int n_alleles, int eaidx, int ref_is_effect,
                           double beta, double eaf) {
    if (int urc = check_usable(c)) return urc;
    if (int arc = check_raw_pl(elem_bytes, n_alleles, eaidx)) return arc;
    if (c->n && !pl) return fail(NPS_E_INVAL, "pl is NULL");
    HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_ds(c);
    if (rc) return rc;
    const size_t bytes = (size_t)elem_bytes * (size_t)(n_alleles * (n_alleles + 1) / 2) * c->n;
    if (c->n) HIP_TRY(c->pl.ensure(pl_slot_bytes(bytes), c->stream.get()));  // (rare: once or twice per context)
    uint32_t slot;
    rc = begin_data_row(c, c->ds, ref_is_effect, NPS_RIE_COUNTS_EFFECT, beta, eaf, &slot);
    if (rc) return rc;
    if (c->n) {
        rc = stage_row(c->pl, c->stream.get(), [&](void *s) { memcpy(s, pl, bytes); }, [&](void *s) -> int {
            ProfScope ps(c, P_DECODE);
            HIP_TRY(launch_decode_pl(c->stream.get(), s, elem_bytes, c->n, n_alleles, eaidx,
                                     c->d_ds.get() + (uint64_t)slot * c->ds_stride_f));
            return NPS_OK;
        });
        if (rc) return rc;
    }
    commit_data_row(c, c->ds, slot);
    return NPS_OK;
}

static int push_gt_typed(nps_ctx *c, const void *gts, int elem_bytes, int ploidy, int eaidx,
                         int ref_is_effect, double beta, double eaf) {
    if (int urc = check_usable(c)) return urc;
    if (c->n && !gts) return fail(NPS_E_INVAL, "gts is NULL");
    if (int arc = check_raw_gt(elem_bytes, ploidy, eaidx, 8)) return arc;
    HIP_TRY(hipSetDevice(c->device));
    if (ploidy > 2)
        return push_gt_polyploid(c, gts, elem_bytes, ploidy, eaidx, ref_is_effect, beta, eaf);
    uint32_t slot;
    int rc = begin_data_row(c, c->gt, ref_is_effect, 0, beta, eaf, &slot);
    if (rc) return rc;
    if (c->n) {
        const size_t bytes = (size_t)elem_bytes * (size_t)ploidy * c->n;
        rc = stage_row(c->raw, c->stream.get(), [&](void *s) { memcpy(s, gts, bytes); }, [&](void *s) -> int {
            ProfScope ps(c, P_DECODE);
            HIP_TRY(launch_decode_gt(c->stream.get(), s, elem_bytes, c->n, ploidy, eaidx,
                                     c->d_codes.get() + (uint64_t)(slot >> 2) * c->stride_words * 4, slot & 3,
                                     c->d_tally.get() + slot));
            return NPS_OK;
        });
        if (rc) return rc;
    }
    commit_data_row(c, c->gt, slot);
    return NPS_OK;
}

extern "C" int nps_push_gt(nps_ctx *c, const int32_t *gts, int ploidy, int eaidx, int ref_is_effect,
                           double beta, double eaf) {
    return push_gt_typed(c, gts, 4, ploidy, eaidx, ref_is_effect, beta, eaf);
}

extern "C" int nps_push_gt_raw(nps_ctx *c, const void *gt, int elem_bytes, int ploidy, int eaidx,
                               int ref_is_effect, double beta, double eaf) {
    return push_gt_typed(c, gt, elem_bytes, ploidy, eaidx, ref_is_effect, beta, eaf);
}

// a row of 2-bit codes, arguments checked: bed_mode -1 = ceil(n/16) words of native codes, else ceil(n/4) bytes of a
// .bed / .pgen row under that code map
static int push_2bit(nps_ctx *c, const void *row, int bed_mode, int ref_is_effect, double beta, double eaf) {
    HIP_TRY(hipSetDevice(c->device));
    uint32_t slot;
    int rc = begin_data_row(c, c->gt, ref_is_effect, 0, beta, eaf, &slot);
    if (rc) return rc;
    if (c->n) {
        rc = stage_row(c->raw, c->stream.get(),
                       [&](void *s) {
                           if (bed_mode < 0)
                               memcpy(s, row, sizeof(uint32_t) * c->n_words);
                           else
                               stage_bed_row(s, (const uint8_t *)row, c->n);
                       },
                       [&](void *s) -> int {
                           ProfScope ps(c, P_TALLY);
                           HIP_TRY(launch_tally_scatter_row(c->stream.get(), (const uint32_t *)s, c->n, bed_mode,
                                                            c->d_codes.get() + (uint64_t)(slot >> 2) * c->stride_words * 4,
                                                            slot & 3, c->d_tally.get() + slot));
                           return NPS_OK;
                       });
        if (rc) return rc;
    }
    commit_data_row(c, c->gt, slot);
    return NPS_OK;
}

extern "C" int nps_push_packed(nps_ctx *c, const uint32_t *row, int ref_is_effect, double beta,
                               double eaf) {
    if (int urc = check_usable(c)) return urc;
    if (c->n && !row) return fail(NPS_E_INVAL, "row is NULL");
    return push_2bit(c, row, -1, ref_is_effect, beta, eaf);
}

extern "C" int nps_push_bed(nps_ctx *c, const uint8_t *bed_row, int effect_is_a1, int ref_is_effect,
                            double beta, double eaf) {
    if (int urc = check_usable(c)) return urc;
    if (c->n && !bed_row) return fail(NPS_E_INVAL, "bed_row is NULL");
    if (effect_is_a1 < 0 || effect_is_a1 > NPS_MAP_PGEN_REF) return fail(NPS_E_INVAL, "bad code map %d", effect_is_a1);
    return push_2bit(c, bed_row, effect_is_a1, ref_is_effect, beta, eaf);
}

// lazily allocate the DS streaming batch.  The ring is built last and is empty after any failure of its own, so a
// built ring says that everything before it succeeded; a call that failed half-way is repeated from the start.
static int ensure_ds(nps_ctx *c) {
    if (c->ds_raw.built()) return NPS_OK;
    c->ds_stride_f = ds_stride_floats(c->n);
    const uint64_t row_bytes = c->ds_stride_f * 4;
    uint64_t cap = (64ull << 20) / row_bytes;
    cap = std::max<uint64_t>(4, std::min<uint64_t>(cap, 1024));
    c->ds.cap = (uint32_t)cap;
    HIP_TRY(c->d_ds.alloc(c->ds_stride_f * cap));
    HIP_TRY(hipMemsetAsync(c->d_ds.get(), 0, row_bytes * cap, c->stream.get()));
    HIP_TRY(c->d_ds_desc.alloc(cap));
    HIP_TRY(c->d_ds_tally.alloc(cap));
    HIP_TRY(c->d_ds_rowp.alloc(cap));
    HIP_TRY(c->d_ds_stats.alloc(cap));
    auto up = [](size_t v) { return (v + 4095) / 4096 * 4096; };
    const size_t sz_desc = up(sizeof(nps_row_desc) * cap), sz_stats = up(sizeof(nps_locus_stat) * cap);
    HIP_TRY(c->h_ds_arena.alloc((sz_desc + sz_stats + 65535) / 65536 * 65536));
    c->ds.h_desc = (nps_row_desc *)c->h_ds_arena.get();
    c->ds.h_stats = (nps_locus_stat *)((char *)c->h_ds_arena.get() + sz_desc);
    HIP_TRY(c->ds_raw.ensure(sizeof(float) * std::max<uint64_t>(c->n, 1), c->stream.get()));
    return NPS_OK;
}

extern "C" int nps_push_ds(nps_ctx *c, const float *ds, int ref_is_effect, double beta, double eaf) {
    if (int urc = check_usable(c)) return urc;
    if (c->n && !ds) return fail(NPS_E_INVAL, "ds is NULL");
    HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_ds(c);
    if (rc) return rc;
    uint32_t slot;
    rc = begin_data_row(c, c->ds, ref_is_effect, 0, beta, eaf, &slot);
    if (rc) return rc;
    if (c->n) {
        rc = stage_row(c->ds_raw, c->stream.get(), [&](void *s) { memcpy(s, ds, sizeof(float) * c->n); }, [&](void *s) -> int {
            HIP_TRY(hipMemcpyAsync(c->d_ds.get() + (uint64_t)slot * c->ds_stride_f, s, sizeof(float) * c->n,
                                   hipMemcpyHostToDevice, c->stream.get()));
            return NPS_OK;
        });
        if (rc) return rc;
    }
    commit_data_row(c, c->ds, slot);
    return NPS_OK;
}

extern "C" int nps_push_locus(nps_ctx *c, int kind, int ref_is_effect, double beta, double eaf) {
    if (int urc = check_usable(c)) return urc;
    if (kind != NPS_ROW_UNCOVERED && kind != NPS_ROW_ABSENT && kind != NPS_ROW_FILTERED)
        return fail(NPS_E_INVAL, "kind %d is not a no-data row kind", kind);
    PendingRow p;
    p.batch_idx = -1;
    p.is_ds = 0;
    host_locus_row(c, kind, ref_is_effect, beta, eaf, &p.host);
    c->pending.push_back(p);
    return NPS_OK;
}

// the device's result block (used rows, status bits) -> pinned host copy; the caller synchronises
static int fetch_result(nps_ctx *c) {
    HIP_TRY(hipMemcpyAsync(c->h_result, c->d_nloci.get(), 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                           c->stream.get()));
    return NPS_OK;
}

// after a stream synchronisation that followed fetch_result: did a bounded wait inside a fused kernel
// expire?  The bit is sticky until nps_reset (the scores of this context are invalid).
static int check_status(nps_ctx *c) {
    if (c->h_result[1] & 1ull)
        return fail(NPS_E_TIMEOUT, "fused kernel: a bounded inter-workgroup wait expired; the scores "
                                   "of this context are invalid (nps_reset and retry in NPS_MODE_TWOPASS)");
    return NPS_OK;
}

extern "C" int nps_flush(nps_ctx *c, nps_locus_stat *stats_out, size_t cap, size_t *n_out) {
    int rc = check_usable(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (stats_out) rc = materialize_resident_stats(c);
    if (rc) return rc;
    rc = run_batch(c);
    if (rc) return rc;
    rc = fetch_result(c);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream.get()));
    rc = check_status(c);
    if (rc) return rc;
    size_t n = 0;
    if (stats_out) {
        while (c->ready_cursor < c->ready.size() && n < cap) stats_out[n++] = c->ready[c->ready_cursor++];
        if (c->ready_cursor == c->ready.size()) {
            c->ready.clear();
            c->ready_cursor = 0;
        }
    }
    if (n_out) *n_out = n;
    return NPS_OK;
}

// nimpress.nim:643-649 on the device, one enqueue and ONE synchronisation: the finish kernel reads
// the device's count of used rows itself, the count and the status bits come back in the same copy
// as (optionally) the scores.
static int finish_common(nps_ctx *c, double offset, double *d_dst, double *h_scores_out,
                         uint64_t *nloci_out, bool normalise = true) {
    int rc = run_batch(c);
    if (rc) return rc;
    if (c->n) {
        ProfScope ps(c, P_REDUCE);
        HIP_TRY(launch_finish(c->stream.get(), c->d_part.get(), c->chunks_used, c->geom.part_chunk_stride, c->n,
                              c->const_sum, c->d_nloci.get(), c->host_nloci, normalise ? 1 : 0, offset, d_dst));
    }
    rc = fetch_result(c);
    if (rc) return rc;
    if (h_scores_out && c->n)
        HIP_TRY(hipMemcpyAsync(h_scores_out, d_dst, sizeof(double) * c->n, hipMemcpyDeviceToHost, c->stream.get()));
    HIP_TRY(hipStreamSynchronize(c->stream.get()));
    rc = check_status(c);
    if (rc) return rc;
    if (nloci_out) *nloci_out = c->host_nloci + c->h_result[0];
    return NPS_OK;
}

extern "C" int nps_finish(nps_ctx *c, double offset, double *scores_out, uint64_t *nloci_out) {
    int rc = check_usable(c);
    if (rc) return rc;
    if (c->n && !scores_out) return fail(NPS_E_INVAL, "scores_out is NULL");
    HIP_TRY(hipSetDevice(c->device));
    return finish_common(c, offset, c->d_scores.get(), scores_out, nloci_out);
}

extern "C" int nps_finish_device(nps_ctx *c, double offset, double *d_scores_out,
                                 uint64_t *nloci_out) {
    int rc = check_usable(c);
    if (rc) return rc;
    if (c->n && !d_scores_out) return fail(NPS_E_INVAL, "d_scores_out is NULL");
    HIP_TRY(hipSetDevice(c->device));
    return finish_common(c, offset, d_scores_out, nullptr, nloci_out);
}

// nps_finish for the kept samples of a set: finish_kernel makes every sample's score as nps_finish does (the same
// arithmetic, so a set that keeps everybody returns nps_finish's bits), the gather takes the kept ones, in cohort
// order, into d_dst[n_kept]
static int check_sampleset(const nps_ctx *c, const nps_sampleset *s) {
    if (!s) return fail(NPS_E_INVAL, "sample set is NULL");
    if (s->device != c->device) return fail(NPS_E_INVAL, "sample set and context are on different devices");
    if (s->n_samples != c->n)
        return fail(NPS_E_INVAL, "sample set has %llu samples, context %llu", (unsigned long long)s->n_samples,
                    (unsigned long long)c->n);
    return NPS_OK;
}

static int finish_subset_common(nps_ctx *c, const nps_sampleset *s, double offset, double *d_dst, double *h_scores_out,
                                uint64_t *nloci_out) {
    int rc = run_batch(c);
    if (rc) return rc;
    {
        ProfScope ps(c, P_REDUCE);
        HIP_TRY(launch_finish(c->stream.get(), c->d_part.get(), c->chunks_used, c->geom.part_chunk_stride, c->n, c->const_sum,
                              c->d_nloci.get(), c->host_nloci, 1, offset, c->d_scores.get()));
        HIP_TRY(launch_subset_gather(c->stream.get(), c->d_scores.get(), c->n, s->d_bits.get(), s->d_prefix.get(), d_dst));
    }
    rc = fetch_result(c);
    if (rc) return rc;
    if (h_scores_out)
        HIP_TRY(hipMemcpyAsync(h_scores_out, d_dst, sizeof(double) * s->n_kept, hipMemcpyDeviceToHost, c->stream.get()));
    HIP_TRY(hipStreamSynchronize(c->stream.get()));
    rc = check_status(c);
    if (rc) return rc;
    if (nloci_out) *nloci_out = c->host_nloci + c->h_result[0];
    return NPS_OK;
}

extern "C" int nps_finish_subset(nps_ctx *c, const nps_sampleset *s, double offset, double *scores_out, uint64_t *nloci_out) {
    int rc = check_usable(c);
    if (rc) return rc;
    rc = check_sampleset(c, s);
    if (rc) return rc;
    if (!scores_out) return fail(NPS_E_INVAL, "scores_out is NULL");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->d_subset_scores.ensure(s->n_kept, c->stream.get()));
    return finish_subset_common(c, s, offset, c->d_subset_scores.get(), scores_out, nloci_out);
}

extern "C" int nps_finish_subset_device(nps_ctx *c, const nps_sampleset *s, double offset, double *d_scores_out,
                                        uint64_t *nloci_out) {
    int rc = check_usable(c);
    if (rc) return rc;
    rc = check_sampleset(c, s);
    if (rc) return rc;
    if (!d_scores_out) return fail(NPS_E_INVAL, "d_scores_out is NULL");
    HIP_TRY(hipSetDevice(c->device));
    return finish_subset_common(c, s, offset, d_scores_out, nullptr, nloci_out);
}

extern "C" int nps_partial_device(nps_ctx *c, double *d_sums_out, uint64_t *nloci_out) {
    int rc = check_usable(c);
    if (rc) return rc;
    if (c->n && !d_sums_out) return fail(NPS_E_INVAL, "d_sums_out is NULL");
    HIP_TRY(hipSetDevice(c->device));
    return finish_common(c, 0.0, d_sums_out, nullptr, nloci_out, false);
}

extern "C" int nps_normalize_device(nps_ctx *c, double *d_sums, uint64_t nloci, double offset) {
    if (!c) return fail(NPS_E_INVAL, "ctx is NULL");
    if (c->n && !d_sums) return fail(NPS_E_INVAL, "d_sums_inout is NULL");
    HIP_TRY(hipSetDevice(c->device));
    if (c->n) {
        // one "chunk" = the reduced sums themselves, in place (every thread reads and writes its own i)
        ProfScope ps(c, P_REDUCE);
        HIP_TRY(launch_finish(c->stream.get(), d_sums, 1, c->n, c->n, 0.0, nullptr, nloci, 1, offset, d_sums));
    }
    HIP_TRY(hipStreamSynchronize(c->stream.get()));
    return NPS_OK;
}

// ------------------------------------------------------------------------------------------
// resident cohort
extern "C" int nps_cohort_create(nps_cohort **out, int device, uint64_t n_samples, uint64_t n_rows,
                                 int format) {
    if (!out) return fail(NPS_E_INVAL, "out is NULL");
    *out = nullptr;
    if (format != NPS_FMT_GT2 && format != NPS_FMT_DS32 && format != NPS_FMT_GT2M && format != NPS_FMT_GT2X &&
        format != NPS_FMT_GT_AUTO && format != NPS_FMT_DS16)
        return fail(NPS_E_INVAL, "unknown cohort format %d", format);
    if (n_samples > 0x7fffffffull) return fail(NPS_E_UNSUPPORTED, "n_samples too large");
    int rc = select_device(device);
    if (rc) return rc;
    if (format == NPS_FMT_GT_AUTO) {
        // The strip layout at every size (round 5).  Where the single-read kernel's grid -- P strips x floor(CUs / P) row
        // teams, all resident -- covers the chip (up to 180 000 samples and 366 593 .. 522 240 on 256 compute units) the
        // tallies are counted in the pass.  Elsewhere (147 strips at 300 000 samples: 147 of 256 compute units; more
        // strips than compute units beyond 522 240) nps_score_cohort[_def] under NPS_MODE_AUTO counts the cohort's
        // tallies ONCE, keeps them with the cohort (nps_cohort_keep_tallies) and scores with the tallies given: an
        // ordinary grid, one read per pass from then on, time independent of the genotypes.  (Until round 4 such sizes got
        // the row layout, whose table-lookup kernel runs at 0.47 .. 0.63 of the roofline depending on the genotypes.)
        format = n_samples < (1ull << 27) ? NPS_FMT_GT2X : NPS_FMT_GT2;
    }
    std::unique_ptr<nps_cohort> owner(new (std::nothrow) nps_cohort);
    nps_cohort *c = owner.get();
    if (!c) return fail(NPS_E_NOMEM, "out of host memory");
    c->device = device;
    c->format = format;
    c->n_samples = n_samples;
    c->n_rows = n_rows;
    c->stride_bytes = format == NPS_FMT_DS32   ? ds_stride_floats(n_samples) * 4
                      : format == NPS_FMT_DS16 ? ds_stride_floats(n_samples) * 2  // (a multiple of 128 bytes)
                                               : stride_words_for(n_samples) * 4;
    const uint64_t rows_alloc = format == NPS_FMT_GT2 ? (n_rows + 3) / 4 * 4 : n_rows;
    uint64_t bytes = std::max<uint64_t>(c->stride_bytes * rows_alloc, 256);
    if (format == NPS_FMT_GT2M) {
        c->stride_bytes = 0;  // not row-major: 1 KiB units of 128 rows x 32 samples
        bytes = std::max<uint64_t>(gt2m_bytes(n_samples, n_rows), 256);
        const uint64_t words = std::max<uint64_t>(gt2m_superblocks(n_rows) * 128, 1);
        if (c->d_row_tally.alloc(words) != hipSuccess ||
            hipMemset(c->d_row_tally.get(), 0, sizeof(unsigned long long) * words) != hipSuccess)
            return fail(NPS_E_NOMEM, "hipMalloc of the row tallies failed");
    }
    if (format == NPS_FMT_GT2X) {
        c->stride_bytes = 0;  // not row-major: strips x superblocks x 1 KiB units
        bytes = std::max<uint64_t>(gt2x_bytes(n_samples, n_rows), 256);
        const uint64_t words = (gt2x_superblocks(n_rows) + 63) / 64;
        c->mx_sb_valid.reset(new (std::nothrow) std::atomic<uint64_t>[std::max<uint64_t>(words, 1)]);
        if (!c->mx_sb_valid) return fail(NPS_E_NOMEM, "out of host memory");
        for (uint64_t w = 0; w < std::max<uint64_t>(words, 1); ++w) c->mx_sb_valid[w].store(0, std::memory_order_relaxed);
    }
    hipError_t e = c->d_data.alloc(bytes);
    if (e != hipSuccess)
        return fail(NPS_E_NOMEM, "allocating %llu bytes for the cohort failed: %s",
                    (unsigned long long)bytes, hipGetErrorString(e));
    e = hipMemset(c->d_data.get(), 0, bytes);
    if (e != hipSuccess) return fail(NPS_E_HIP, "hipMemset failed: %s", hipGetErrorString(e));
    *out = owner.release();
    return NPS_OK;
}

extern "C" uint64_t nps_cohort_row_stride(const nps_cohort *c) { return c ? c->stride_bytes : 0; }
extern "C" uint64_t nps_cohort_n_rows(const nps_cohort *c) { return c ? c->n_rows : 0; }
extern "C" int nps_cohort_format(const nps_cohort *c) { return c ? c->format : -1; }

extern "C" void nps_cohort_destroy(nps_cohort *c) { delete c; }

// back to the plain layout (before rows are written into an optimised cohort); the transform is its own inverse
static int cohort_unoptimize(nps_cohort *c) {
    if (!c->optimized) return NPS_OK;
    hipError_t e = launch_cohort_parity(nullptr, (uint32_t *)c->d_data.get(), c->stride_bytes / 4, c->n_samples, c->n_rows);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(NPS_E_HIP, "cohort re-ordering failed: %s", hipGetErrorString(e));
    c->optimized = false;
    return NPS_OK;
}

extern "C" int nps_cohort_optimize(nps_cohort *c) {
    if (!c) return fail(NPS_E_INVAL, "cohort is NULL");
    if (c->format != NPS_FMT_GT2 || c->optimized || c->n_rows == 0 || c->n_samples == 0) return NPS_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());  // no scoring kernel may still be reading the rows rewritten here
    hipError_t e = launch_cohort_parity(nullptr, (uint32_t *)c->d_data.get(), c->stride_bytes / 4, c->n_samples, c->n_rows);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(NPS_E_HIP, "cohort optimisation failed: %s", hipGetErrorString(e));
    c->optimized = true;
    return NPS_OK;
}

static int check_range(const nps_cohort *c, uint64_t row0, uint64_t nrows) {
    if (!c) return fail(NPS_E_INVAL, "cohort is NULL");
    if (row0 > c->n_rows || nrows > c->n_rows - row0)
        return fail(NPS_E_INVAL, "rows [%llu,+%llu) outside cohort of %llu rows",
                    (unsigned long long)row0, (unsigned long long)nrows,
                    (unsigned long long)c->n_rows);
    return NPS_OK;
}

// GT2 rows <-> the group-interleaved device layout, through a host buffer of whole groups
static int gt2_transfer(const nps_cohort *c, uint64_t row0, uint64_t nrows, void *host_rows,
                        size_t host_stride, bool to_device) {
    const uint64_t n_words = words_for(c->n_samples), sw = c->stride_bytes / 4;
    if (row0 & 3) return fail(NPS_E_INVAL, "row0 must be a multiple of 4 for 2-bit cohorts");
    const uint64_t chunk_groups = std::max<uint64_t>(1, (64ull << 20) / (sw * 16));
    std::vector<uint32_t> buf;
    // (more than one chunk: tests/test_gpu_seams.py seam_tall_row_upload_and_download_cross_their_chunks)
    for (uint64_t r = 0; r < nrows; r += chunk_groups * 4) {
        const uint64_t k = std::min<uint64_t>(chunk_groups * 4, nrows - r);  // rows in this chunk
        const uint64_t groups = (k + 3) / 4;
        char *dev = (char *)c->d_data.get() + ((row0 + r) >> 2) * sw * 16;
        buf.assign(groups * sw * 4, 0u);
        if (!to_device) {
            HIP_TRY(hipMemcpy(buf.data(), dev, groups * sw * 16, hipMemcpyDeviceToHost));
            if (c->optimized)  // parity layout -> plain, on the copy
                for (uint64_t x = 0; x < groups * sw; ++x) {
                    uint32_t *q = buf.data() + x * 4;
                    q[0] = parity_fix(q[0], q[1], q[2], q[3]);
                }
        }
        for (uint64_t j = 0; j < k; ++j) {
            uint32_t *hrow = (uint32_t *)((char *)host_rows + (r + j) * host_stride);
            uint32_t *g = buf.data() + (j >> 2) * sw * 4 + (j & 3);
            if (to_device)
                for (uint64_t w = 0; w < n_words; ++w) g[w * 4] = word_to_planes(hrow[w]);
            else
                for (uint64_t w = 0; w < n_words; ++w) hrow[w] = word_from_planes(g[w * 4]);
        }
        // rows of a last partial group that are not part of this upload become zero
        if (to_device)
            HIP_TRY(hipMemcpy(dev, buf.data(), groups * sw * 16, hipMemcpyHostToDevice));
    }
    return NPS_OK;
}

// k host rows of `width` bytes -> staging rows `pitch` bytes apart.  Short rows whose width or stride is no multiple of 4
// (.bed / .pgen rows of a few dozen samples) cost hipMemcpy2D microseconds EACH (a minute for eight million rows): those are
// laid out at the pitch on the host, padding zero, and go over in one copy.
static hipError_t stage_host_rows(void *d_stage, size_t pitch, const char *host, size_t host_stride, size_t width, uint64_t k,
                                  std::vector<char> &repitched) {
    if (((width | host_stride) & 3) == 0 || pitch > 4096)
        return hipMemcpy2D(d_stage, pitch, host, host_stride, width, k, hipMemcpyHostToDevice);
    repitched.assign(k * pitch, 0);
    for (uint64_t j = 0; j < k; ++j) memcpy(repitched.data() + j * pitch, host + j * host_stride, width);
    return hipMemcpy(d_stage, repitched.data(), k * pitch, hipMemcpyHostToDevice);
}

// rows of a host buffer -> staging on the device -> interleave (and, for .bed rows, recode) kernel.
// width = bytes of one source row; bed_mode: nullptr (native codes) or per-row effect-is-A1 flags.
static int gt2_upload(nps_cohort *c, uint64_t row0, uint64_t nrows, const void *host_rows,
                      size_t host_stride, size_t width, const uint8_t *bed_mode) {
    if (row0 & 3) return fail(NPS_E_INVAL, "row0 must be a multiple of 4 for 2-bit cohorts");
    const uint64_t sw = c->stride_bytes / 4;  // word columns per group in the cohort
    const uint64_t src_stride_words = sw;     // staging rows padded the same way (zero filled)
    uint64_t chunk = std::max<uint64_t>(4, (256ull << 20) / (src_stride_words * 4)) / 4 * 4;
    chunk = std::min<uint64_t>(chunk, 4ull * 65535);
    chunk = std::min<uint64_t>(chunk, (nrows + 3) / 4 * 4);
    DevBuf<uint32_t> d_stage;
    DevBuf<uint8_t> d_mode;
    HIP_TRY(d_stage.alloc(chunk * src_stride_words));
    if (bed_mode) HIP_TRY(d_mode.alloc(chunk));
    std::vector<char> repitched;
    // (more than one chunk: tests/test_gpu_seams.py seam_tall_row_upload_*, seam_wide_row_layout_upload_and_download)
    for (uint64_t r = 0; r < nrows; r += chunk) {
        const uint64_t k = std::min(chunk, nrows - r);
        HIP_TRY(hipMemsetAsync(d_stage.get(), 0, chunk * src_stride_words * 4, nullptr));
        HIP_TRY(stage_host_rows(d_stage.get(), src_stride_words * 4, (const char *)host_rows + r * host_stride, host_stride,
                                width, k, repitched));
        if (bed_mode) HIP_TRY(hipMemcpy(d_mode.get(), bed_mode + r, k, hipMemcpyHostToDevice));
        HIP_TRY(launch_interleave_rows(nullptr, d_stage.get(), src_stride_words, k, c->n_samples, d_mode.get(),
                                       (uint32_t *)(c->d_data.get() + ((row0 + r) >> 2) * sw * 16), sw));
        HIP_TRY(hipDeviceSynchronize());
    }
    return NPS_OK;
}

// NPS_FMT_GT2X: units -> plain rows (C-ABI order and codes), through a device staging buffer of whole superblocks
static int gt2x_download(const nps_cohort *c, uint64_t row0, uint64_t nrows, void *host_rows, size_t host_stride) {
    const uint64_t n_words = words_for(c->n_samples), sw = (n_words + 3) / 4 * 4;
    uint64_t chunk = std::max<uint64_t>(128, (256ull << 20) / (sw * 4) / 128 * 128);
    chunk = std::min<uint64_t>(chunk, 128ull * 65535);  // one launch_gt2x_to_rows takes 65 535 superblocks
    DevBuf<uint32_t> d_stage;
    HIP_TRY(d_stage.alloc(std::min(chunk, (nrows + 127) / 128 * 128) * sw));
    // (more than one chunk: tests/test_gpu_seams.py seam_tall_strip_upload_in_one_call, seam_wide_strip_layout_fill_and_download)
    for (uint64_t r = 0; r < nrows; r += chunk) {
        const uint64_t k = std::min(chunk, nrows - r);
        HIP_TRY(launch_gt2x_to_rows(nullptr, c->d_data.get(), c->n_samples, c->n_rows, row0 + r, k, d_stage.get(), sw));
        HIP_TRY(hipMemcpy2D((char *)host_rows + r * host_stride, host_stride, d_stage.get(), sw * 4, n_words * 4, k,
                            hipMemcpyDeviceToHost));
    }
    return NPS_OK;
}

// NPS_FMT_GT2X: host rows -> staging on the device -> units AND the rows' tally words (fill_gt2x_kernel), whole
// superblocks at a time.  width = bytes of one source row; code_map: nullptr (rows of NPS_CODE_* codes) or a NPS_MAP_* per
// row (.bed / .pgen rows).  The superblocks written are invalid from the start of the call and valid again -- with the new
// rows' tallies -- once every launch has completed; superblocks the call does not touch keep their state.
static int gt2x_fill(nps_cohort *c, uint64_t row0, uint64_t nrows, const void *host_rows, size_t host_stride, size_t width,
                     const uint8_t *code_map) {
    if (row0 & 127) return fail(NPS_E_INVAL, "row0 must be a multiple of 128 for NPS_FMT_GT2X cohorts");
    if (c->n_samples >= (1ull << 27)) return fail(NPS_E_UNSUPPORTED, "more than 2^27 samples");
    const uint64_t n_words = words_for(c->n_samples), sw = (n_words + 3) / 4 * 4;
    uint64_t chunk = std::max<uint64_t>(128, (256ull << 20) / (sw * 4) / 128 * 128);
    chunk = std::min<uint64_t>(chunk, 128ull * 32768);
    mx_tallies_rewrite(c, row0, nrows);
    std::lock_guard<std::mutex> lk(c->tally_mutex);
    HIP_TRY(mx_tallies_alloc(c));
    const uint64_t sb0 = row0 >> 7, n_sb = (nrows + 127) / 128;
    DevBuf<uint32_t> d_stage;
    DevBuf<uint8_t> d_map;
    HIP_TRY(d_stage.alloc(std::min(chunk, n_sb * 128) * sw));
    if (code_map) HIP_TRY(d_map.alloc(std::min(chunk, nrows)));
    std::vector<char> repitched;
    HIP_TRY(hipMemsetAsync(c->d_mx_row_tally.get() + sb0 * 128, 0, sizeof(unsigned long long) * n_sb * 128, nullptr));
    // (more than one chunk: tests/test_gpu_seams.py seam_tall_strip_upload*_in_one_call, seam_wide_strip_layout_fill_and_download)
    for (uint64_t r = 0; r < nrows; r += chunk) {
        const uint64_t k = std::min(chunk, nrows - r);
        HIP_TRY(stage_host_rows(d_stage.get(), sw * 4, (const char *)host_rows + r * host_stride, host_stride, width, k,
                                repitched));
        if (code_map) HIP_TRY(hipMemcpy(d_map.get(), code_map + r, k, hipMemcpyHostToDevice));
        HIP_TRY(launch_fill_gt2x_rows(nullptr, d_stage.get(), sw, d_map.get(), c->n_samples, c->n_rows, row0 + r, k,
                                      c->d_data.get(), c->d_mx_row_tally.get()));
        HIP_TRY(hipDeviceSynchronize());
    }
    mx_tallies_mark(c, sb0, n_sb, true);
    return NPS_OK;
}

extern "C" int nps_cohort_upload_bed(nps_cohort *c, uint64_t row0, uint64_t nrows, const uint8_t *bed_rows,
                                     size_t row_stride_bytes, const uint8_t *effect_is_a1) {
    int rc = check_range(c, row0, nrows);
    if (rc) return rc;
    if (c->format != NPS_FMT_GT2 && c->format != NPS_FMT_GT2X)
        return fail(NPS_E_INVAL, ".bed rows need a 2-bit (NPS_FMT_GT2 or NPS_FMT_GT2X) cohort");
    if (c->format == NPS_FMT_GT2X && (row0 & 127))
        return fail(NPS_E_INVAL, "row0 must be a multiple of 128 for NPS_FMT_GT2X cohorts");
    const size_t width = (size_t)((c->n_samples + 3) / 4);
    if (nrows == 0 || width == 0) return NPS_OK;
    if (!bed_rows || !effect_is_a1 || row_stride_bytes < width)
        return fail(NPS_E_INVAL, "bad .bed buffer / stride / flags");
    for (uint64_t r = 0; r < nrows; ++r)
        if (effect_is_a1[r] > NPS_MAP_PGEN_REF) return fail(NPS_E_INVAL, "row %llu: bad code map %d", (unsigned long long)r, (int)effect_is_a1[r]);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());  // no scoring kernel may still be reading the rows replaced here
    if (c->format == NPS_FMT_GT2X) return gt2x_fill(c, row0, nrows, bed_rows, row_stride_bytes, width, effect_is_a1);
    rc = cohort_unoptimize(c);
    if (rc) return rc;
    return gt2_upload(c, row0, nrows, bed_rows, row_stride_bytes, width, effect_is_a1);
}

// one row of a NPS_FMT_GT2 cohort from the buffer a VCF/BCF record holds, decoded on the device (the resident form of
// nps_push_gt_raw / nps_push_bed: same kernels, the cohort is the destination)
// (format: what the pushed row decodes to -- 2-bit codes, or for nps_cohort_push_pl float32 dosages)
static int cohort_push_prepare(nps_cohort *c, uint64_t row, size_t bytes, int format = NPS_FMT_GT2) {
    if (!c) return fail(NPS_E_INVAL, "cohort is NULL");
    if (c->format != format)
        return format == NPS_FMT_GT2 ? fail(NPS_E_UNSUPPORTED, "rows are pushed into NPS_FMT_GT2 cohorts only")
                                     : fail(NPS_E_UNSUPPORTED, "FORMAT/PL rows are pushed into NPS_FMT_DS32 cohorts only");
    if (row >= c->n_rows) return fail(NPS_E_INVAL, "row %llu outside cohort of %llu rows", (unsigned long long)row,
                                      (unsigned long long)c->n_rows);
    HIP_TRY(hipSetDevice(c->device));
    if (!c->push_stream.get()) {
        HIP_TRY(hipDeviceSynchronize());  // whatever wrote or read the cohort before
        int rc = cohort_unoptimize(c);
        if (rc) return rc;
        HIP_TRY(c->push_stream.create());
    }
    if (format == NPS_FMT_GT2 && !c->d_push_tally.get()) HIP_TRY(c->d_push_tally.alloc(256 / sizeof(unsigned long long)));
    if (c->optimized) {
        HIP_TRY(hipDeviceSynchronize());
        int rc = cohort_unoptimize(c);
        if (rc) return rc;
    }
    HIP_TRY(c->push.ensure(bytes, c->push_stream.get()));
    return NPS_OK;
}

extern "C" int nps_cohort_push_gt_raw(nps_cohort *c, uint64_t row, const void *gt, int elem_bytes, int ploidy,
                                      int eaidx) {
    if (int arc = check_raw_gt(elem_bytes, ploidy, eaidx, 2)) return arc;
    if (c && c->n_samples && !gt) return fail(NPS_E_INVAL, "gt is NULL");
    const size_t bytes = c ? (size_t)elem_bytes * (size_t)ploidy * c->n_samples : 0;
    int rc = cohort_push_prepare(c, row, std::max<size_t>(bytes, 16));
    if (rc) return rc;
    if (c->n_samples == 0) return NPS_OK;
    const uint64_t sw = c->stride_bytes / 4;
    return stage_row(c->push, c->push_stream.get(), [&](void *s) { memcpy(s, gt, bytes); }, [&](void *s) -> int {
        HIP_TRY(launch_decode_gt(c->push_stream.get(), s, elem_bytes, c->n_samples, ploidy, eaidx,
                                 (uint32_t *)c->d_data.get() + (row >> 2) * sw * 4, (int)(row & 3), c->d_push_tally.get()));
        return NPS_OK;
    });
}

extern "C" int nps_cohort_push_bed(nps_cohort *c, uint64_t row, const uint8_t *bed_row, int effect_is_a1) {
    if (c && c->n_samples && !bed_row) return fail(NPS_E_INVAL, "bed_row is NULL");
    if (effect_is_a1 < 0 || effect_is_a1 > NPS_MAP_PGEN_REF) return fail(NPS_E_INVAL, "bad code map %d", effect_is_a1);
    const size_t bytes = c ? (size_t)((c->n_samples + 3) / 4) : 0;
    int rc = cohort_push_prepare(c, row, (bytes + 3) / 4 * 4 + 16);
    if (rc) return rc;
    if (c->n_samples == 0) return NPS_OK;
    const uint64_t sw = c->stride_bytes / 4;
    return stage_row(c->push, c->push_stream.get(), [&](void *s) { stage_bed_row(s, bed_row, c->n_samples); }, [&](void *s) -> int {
        HIP_TRY(launch_tally_scatter_row(c->push_stream.get(), (const uint32_t *)s, c->n_samples, effect_is_a1,
                                         (uint32_t *)c->d_data.get() + (row >> 2) * sw * 4, (int)(row & 3),
                                         c->d_push_tally.get()));
        return NPS_OK;
    });
}

// One row of a NPS_FMT_DS32 cohort from the FORMAT/PL vector of a record (the resident form of nps_push_pl: same kernel,
// the cohort is the destination).  The values written are in [0, 2] or NaN: the cohort's out-of-range state is untouched.
extern "C" int nps_cohort_push_pl(nps_cohort *c, uint64_t row, const void *pl, int elem_bytes, int n_alleles, int eaidx) {
    if (int arc = check_raw_pl(elem_bytes, n_alleles, eaidx)) return arc;
    if (c && c->n_samples && !pl) return fail(NPS_E_INVAL, "pl is NULL");
    const size_t bytes = c ? (size_t)elem_bytes * (size_t)(n_alleles * (n_alleles + 1) / 2) * c->n_samples : 0;
    int rc = cohort_push_prepare(c, row, std::max<size_t>(pl_slot_bytes(bytes), 16), NPS_FMT_DS32);
    if (rc) return rc;
    if (c->n_samples == 0) return NPS_OK;
    return stage_row(c->push, c->push_stream.get(), [&](void *s) { memcpy(s, pl, bytes); }, [&](void *s) -> int {
        HIP_TRY(launch_decode_pl(c->push_stream.get(), s, elem_bytes, c->n_samples, n_alleles, eaidx,
                                 (float *)(c->d_data.get() + row * c->stride_bytes)));
        return NPS_OK;
    });
}

// NPS_FMT_DS16 <-> float32 rows of the host, through a float32 staging buffer of at most 256 MiB.  Upload: a row that holds
// a value which is not the value of a code (a decimal with at most four places in [0, 2], as float32) is REFUSED -- the
// format is lossless or it is not used; the rows of the range are undefined after a refusal.
static int ds16_transfer(nps_cohort *c, uint64_t row0, uint64_t nrows, void *host_rows, size_t host_stride, bool upload) {
    const uint64_t stride_f = ds_stride_floats(c->n_samples), stride_e = c->stride_bytes / 2;
    const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(nrows, (256ull << 20) / (stride_f * 4)));
    DevBuf<float> d_stage;
    DevBuf<unsigned char> d_bad;
    HIP_TRY(d_stage.alloc(chunk * stride_f));
    HIP_TRY(d_bad.alloc(chunk));
    std::vector<unsigned char> bad(chunk);
    long long first_bad = -1;
    // (more than one chunk: tests/test_gpu_seams.py seam_ds16_staging_chunks_and_the_row_an_error_names)
    for (uint64_t r = 0; r < nrows && first_bad < 0; r += chunk) {
        const uint64_t k = std::min(chunk, nrows - r);
        uint16_t *rows = (uint16_t *)c->d_data.get() + (row0 + r) * stride_e;
        char *host = (char *)host_rows + r * host_stride;
        if (upload) {
            HIP_TRY(hipMemcpy2D(d_stage.get(), stride_f * 4, host, host_stride, c->n_samples * 4, k, hipMemcpyHostToDevice));
            HIP_TRY(launch_ds16_pack(nullptr, d_stage.get(), stride_f, c->n_samples, k, rows, stride_e, d_bad.get()));
            HIP_TRY(hipMemcpy(bad.data(), d_bad.get(), k, hipMemcpyDeviceToHost));
            for (uint64_t j = 0; j < k; ++j)
                if (bad[j]) {
                    first_bad = (long long)(row0 + r + j);
                    break;
                }
        } else {
            HIP_TRY(launch_ds16_unpack(nullptr, rows, stride_e, c->n_samples, k, d_stage.get(), stride_f));
            HIP_TRY(hipMemcpy2D(host, host_stride, d_stage.get(), stride_f * 4, c->n_samples * 4, k, hipMemcpyDeviceToHost));
        }
    }
    if (first_bad >= 0)
        return fail(NPS_E_UNSUPPORTED, "row %lld holds a FORMAT/DS value that is not a decimal with at most four places in "
                    "[0, 2]: NPS_FMT_DS16 stores such values only (losslessly); use a NPS_FMT_DS32 cohort", first_bad);
    return NPS_OK;
}

extern "C" int nps_cohort_upload(nps_cohort *c, uint64_t row0, uint64_t nrows, const void *host_rows,
                                 size_t host_stride) {
    int rc = check_range(c, row0, nrows);
    if (rc) return rc;
    if (c->format == NPS_FMT_GT2M)
        return fail(NPS_E_UNSUPPORTED, "NPS_FMT_GT2M cohorts are filled by nps_cohort_convert (from a "
                                       "NPS_FMT_GT2 cohort) or by the synthetic generator");
    const bool ds_any = c->format == NPS_FMT_DS32 || c->format == NPS_FMT_DS16;  // (both take and give float32 rows)
    const size_t width = ds_any ? c->n_samples * 4 : words_for(c->n_samples) * 4;
    if (nrows == 0 || width == 0) return NPS_OK;
    if (!host_rows || host_stride < width) return fail(NPS_E_INVAL, "bad host buffer / stride");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());  // no scoring kernel may still be reading the rows replaced here
    if (c->format == NPS_FMT_DS16) return ds16_transfer(c, row0, nrows, const_cast<void *>(host_rows), host_stride, true);
    if (c->format == NPS_FMT_GT2) {
        rc = cohort_unoptimize(c);
        if (rc) return rc;
        return gt2_upload(c, row0, nrows, host_rows, host_stride, width, nullptr);
    }
    if (c->format == NPS_FMT_GT2X) return gt2x_fill(c, row0, nrows, host_rows, host_stride, width, nullptr);
    HIP_TRY(hipMemcpy2D((char *)c->d_data.get() + row0 * c->stride_bytes, c->stride_bytes, host_rows,
                        host_stride, width, nrows, hipMemcpyHostToDevice));
    // the range of a dosage, row by row, where the rows now lie (one read at upload time, none when scoring)
    DevBuf<unsigned char> d_bad;
    HIP_TRY(d_bad.alloc(nrows));
    std::vector<unsigned char> bad(nrows);
    HIP_TRY(launch_ds_range_check(nullptr, (const float *)c->d_data.get() + row0 * (c->stride_bytes / 4), c->stride_bytes / 4,
                                  c->n_samples, nrows, d_bad.get()));
    HIP_TRY(hipMemcpy(bad.data(), d_bad.get(), nrows, hipMemcpyDeviceToHost));
    if (c->ds_row_bad.size() != c->n_rows) c->ds_row_bad.assign(c->n_rows, 0);
    for (uint64_t r = 0; r < nrows; ++r) {
        c->ds_bad_rows += (uint64_t)bad[r] - (uint64_t)c->ds_row_bad[row0 + r];
        c->ds_row_bad[row0 + r] = bad[r];
    }
    return NPS_OK;
}

extern "C" int nps_cohort_download(const nps_cohort *c, uint64_t row0, uint64_t nrows,
                                   void *host_rows, size_t host_stride) {
    int rc = check_range(c, row0, nrows);
    if (rc) return rc;
    if (c->format == NPS_FMT_GT2M) return fail(NPS_E_UNSUPPORTED, "NPS_FMT_GT2M cohorts cannot be downloaded");
    const size_t width = c->format == NPS_FMT_DS32 || c->format == NPS_FMT_DS16 ? c->n_samples * 4 : words_for(c->n_samples) * 4;
    if (nrows == 0 || width == 0) return NPS_OK;
    if (!host_rows || host_stride < width) return fail(NPS_E_INVAL, "bad host buffer / stride");
    HIP_TRY(hipSetDevice(c->device));
    { int qrc = cohort_quiesce(c); if (qrc) return qrc; }
    if (c->format == NPS_FMT_DS16) return ds16_transfer(const_cast<nps_cohort *>(c), row0, nrows, host_rows, host_stride, false);
    if (c->format == NPS_FMT_GT2) return gt2_transfer(c, row0, nrows, host_rows, host_stride, false);
    if (c->format == NPS_FMT_GT2X) return gt2x_download(c, row0, nrows, host_rows, host_stride);
    HIP_TRY(hipMemcpy2D(host_rows, host_stride, (const char *)c->d_data.get() + row0 * c->stride_bytes,
                        c->stride_bytes, width, nrows, hipMemcpyDeviceToHost));
    return NPS_OK;
}

extern "C" int nps_cohort_synth_rows(nps_cohort *c, uint64_t row0, uint64_t nrows, uint64_t gen_row0,
                                     uint64_t seed, const uint32_t *t_het, const uint32_t *t_hom,
                                     const uint32_t *t_miss) {
    int rc = check_range(c, row0, nrows);
    if (rc) return rc;
    if (nrows == 0) return NPS_OK;
    if (!t_het || !t_hom || !t_miss) return fail(NPS_E_INVAL, "threshold arrays are NULL");
    if (c->format == NPS_FMT_GT2 && (row0 & 3))
        return fail(NPS_E_INVAL, "row0 must be a multiple of 4 for 2-bit cohorts");
    if ((c->format == NPS_FMT_GT2M || c->format == NPS_FMT_GT2X) && (row0 & 127))
        return fail(NPS_E_INVAL, "row0 must be a multiple of 128 for NPS_FMT_GT2M / NPS_FMT_GT2X cohorts");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());  // no scoring kernel may still be reading the rows replaced here
    // (a strip cohort's generator counts nothing, on purpose: the superblocks it writes carry no tallies afterwards and a
    //  synthetic cohort is scored as it always was -- counted in the pass, or once by the first pass that wants them kept)
    mx_tallies_rewrite(c, row0, nrows);
    rc = cohort_unoptimize(c);
    if (rc) return rc;
    DevBuf<uint32_t> d_thr;  // the three threshold arrays, one after the other
    HIP_TRY(d_thr.alloc(3 * nrows));
    uint32_t *const d_t = d_thr.get();
    HIP_TRY(hipMemcpy(d_t, t_het, sizeof(uint32_t) * nrows, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_t + nrows, t_hom, sizeof(uint32_t) * nrows, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_t + 2 * nrows, t_miss, sizeof(uint32_t) * nrows, hipMemcpyHostToDevice));
    const uint64_t step = 32768;
    hipError_t e = hipSuccess;
    for (uint64_t r = 0; e == hipSuccess && r < nrows; r += step) {
        const uint64_t k = std::min(step, nrows - r);
        if (c->format == NPS_FMT_GT2M)
            e = launch_synth_gt2m(nullptr, c->d_data.get(), c->n_samples, row0 + r, gen_row0 + r, k, seed, d_t + r,
                                  d_t + nrows + r, d_t + 2 * nrows + r, c->d_row_tally.get());
        else if (c->format == NPS_FMT_GT2X)
            e = launch_synth_gt2x(nullptr, c->d_data.get(), c->n_samples, c->n_rows, row0 + r, gen_row0 + r, k, seed, d_t + r,
                                  d_t + nrows + r, d_t + 2 * nrows + r);
        else if (c->format == NPS_FMT_DS16)
            e = launch_synth_ds16(nullptr, (uint16_t *)c->d_data.get(), c->stride_bytes / 2, c->n_samples, row0 + r, gen_row0 + r, k,
                                  seed, d_t + r, d_t + nrows + r, d_t + 2 * nrows + r);
        else if (c->format == NPS_FMT_DS32)
            e = launch_synth_ds(nullptr, (float *)c->d_data.get(), c->stride_bytes / 4, c->n_samples,
                                row0 + r, gen_row0 + r, k, seed, d_t + r, d_t + nrows + r, d_t + 2 * nrows + r);
        else
            e = launch_synth_gt(nullptr, (uint32_t *)c->d_data.get(), c->stride_bytes / 4, c->n_samples,
                                row0 + r, gen_row0 + r, k, seed, d_t + r, d_t + nrows + r, d_t + 2 * nrows + r);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(NPS_E_HIP, "synthetic fill failed: %s", hipGetErrorString(e));
    if (c->format == NPS_FMT_DS32 && c->ds_bad_rows)  // the generator clips to [0, 2]: these rows are in range now
        for (uint64_t r = row0; r < row0 + nrows && r < c->ds_row_bad.size(); ++r) {
            c->ds_bad_rows -= c->ds_row_bad[r];
            c->ds_row_bad[r] = 0;
        }
    return NPS_OK;
}

extern "C" int nps_cohort_synth(nps_cohort *c, uint64_t row0, uint64_t nrows, uint64_t seed,
                                const uint32_t *t_het, const uint32_t *t_hom, const uint32_t *t_miss) {
    return nps_cohort_synth_rows(c, row0, nrows, row0, seed, t_het, t_hom, t_miss);
}

// ------------------------------------------------------------------------------------------
// score definitions kept on the device
struct nps_scoredef {
    int device = 0;
    uint64_t n_desc = 0;
    uint64_t m = 0;                       // PRESENT rows (consume cohort rows)
    std::vector<nps_row_desc> host_rows;  // rows without genotype data, in order
    std::vector<int64_t> data_index;      // per desc: >= 0 index among PRESENT rows, -1 host row
    DevBuf<nps_row_desc> d_desc;          // [m] PRESENT rows, compact
    // NPS_FMT_GT2X runs: the largest |beta| (4 + max(2, 2 |eaf|)) over the PRESENT rows with finite numbers: the
    // fixed-point scale 2^F of fused_mx_kernel keeps every weight below 2^56
    double mx_bound = 0.0;
    // ... and when the definition's weights span more than 2^30 (a sample that carries only its small-beta rows would see
    // the quantisation of the largest one): magnitude bands of 2^30, each a copy of the PRESENT rows with beta = 0
    // outside the band, scored one pass per band with the band's own scale (empty: one band, d_desc itself)
    struct MxBand {
        double bound = 0.0;
        DevBuf<nps_row_desc> d_desc;
    };
    std::vector<MxBand> mx_bands;
    // ... and the PRESENT rows those kernels cannot carry (mx_special): their indices among the PRESENT rows, ascending,
    // and their descriptors as given.  d_mx_desc is d_desc with these rows at beta = eaf = 0 (null: no special row);
    // after the fixed-point pass mx_special_pass adds their products in IEEE double.
    std::vector<uint64_t> special;
    DevBuf<nps_row_desc> d_special;
    DevBuf<nps_row_desc> d_mx_desc;

    ~nps_scoredef() { (void)hipSetDevice(device); }
};

// n row descriptors of the host, on the device
static hipError_t upload_desc(DevBuf<nps_row_desc> &d, const nps_row_desc *rows, uint64_t n) {
    const hipError_t e = d.alloc(n);
    return e != hipSuccess ? e : hipMemcpy(d.get(), rows, sizeof(nps_row_desc) * n, hipMemcpyHostToDevice);
}
constexpr int kMxBandBits = 30, kMxMaxBands = 8;

// A PRESENT row the fixed-point kernels of NPS_FMT_GT2X cohorts cannot carry: a non-finite beta (0 x inf is NaN, every
// other dosage +-inf), an infinite eaf (the products of an imputed dosage are +-inf, and the kernels keep one NaN flag per
// row), or a weight bound |beta| (4 + max(2, 2 |eaf|)) outside [2^-900, 2^1000): beyond the fixed-point scale 2^F,
// |F| <= 1000, and beyond the overflow of the bound itself.  A NaN eaf is not special: its products are NaN.
static bool mx_special(const nps_row_desc &r, double *bound) {
    *bound = 0.0;
    if (!std::isfinite(r.beta) || std::isinf(r.eaf)) return true;
    const double ie = std::isfinite(r.eaf) ? std::max(2.0, 2.0 * std::fabs(r.eaf)) : 2.0;
    *bound = std::fabs(r.beta) * (4.0 + ie);
    return r.beta != 0.0 && !(*bound >= 0x1p-900 && *bound < 0x1p1000);
}

extern "C" int nps_scoredef_create(nps_scoredef **out, int device, const nps_row_desc *rows,
                                   uint64_t n_desc) {
    if (!out) return fail(NPS_E_INVAL, "out is NULL");
    *out = nullptr;
    if (n_desc && !rows) return fail(NPS_E_INVAL, "rows is NULL");
    int rc = select_device(device);
    if (rc) return rc;
    std::unique_ptr<nps_scoredef> owner(new (std::nothrow) nps_scoredef);
    nps_scoredef *d = owner.get();
    if (!d) return fail(NPS_E_NOMEM, "out of host memory");
    d->device = device;
    d->n_desc = n_desc;
    std::vector<nps_row_desc> data;
    data.reserve(n_desc);
    d->data_index.resize(n_desc);
    for (uint64_t j = 0; j < n_desc; ++j) {
        const nps_row_desc &r = rows[j];
        if (r.kind == NPS_ROW_PRESENT) {
            d->data_index[j] = (int64_t)data.size();
            double bound = 0.0;
            if (mx_special(r, &bound))
                d->special.push_back(data.size());
            else
                d->mx_bound = std::max(d->mx_bound, bound);
            data.push_back(r);
        } else if (r.kind == NPS_ROW_UNCOVERED || r.kind == NPS_ROW_ABSENT ||
                   r.kind == NPS_ROW_FILTERED) {
            d->data_index[j] = -1;
            d->host_rows.push_back(r);
        } else {
            return fail(NPS_E_INVAL, "row %llu: bad kind %d", (unsigned long long)j, r.kind);
        }
    }
    d->m = data.size();
    if (d->m > 0xfffffff0ull) return fail(NPS_E_UNSUPPORTED, "too many rows");
    if (d->m) {
        HIP_TRY(upload_desc(d->d_desc, data.data(), d->m));
        if (!d->special.empty()) {
            const uint64_t k = d->special.size();
            std::vector<nps_row_desc> sp(k);
            for (uint64_t i = 0; i < k; ++i) {
                sp[i] = data[d->special[i]];
                data[d->special[i]].beta = 0.0;  // (from here on `data` is the fixed-point copy)
                data[d->special[i]].eaf = 0.0;
            }
            HIP_TRY(upload_desc(d->d_special, sp.data(), k));
            HIP_TRY(upload_desc(d->d_mx_desc, data.data(), d->m));
        }
        // magnitude bands for the fixed-point kernel (north star: 1e-6 RELATIVE for every sample, also one whose only
        // rows are the definition's smallest): band b holds the rows with bound 2^-30(b+1) < v <= bound 2^-30b
        std::vector<int> band(d->m, 0);
        int n_bands = 1;
        if (d->mx_bound > 0.0) {
            for (uint64_t j = 0; j < d->m; ++j) {
                const nps_row_desc &r = data[j];
                if (!std::isfinite(r.beta) || r.beta == 0.0) continue;
                const double ie = std::isfinite(r.eaf) ? std::max(2.0, 2.0 * std::fabs(r.eaf)) : 2.0;
                int e_top = 0, e_v = 0;
                (void)std::frexp(d->mx_bound, &e_top);
                (void)std::frexp(std::fabs(r.beta) * (4.0 + ie), &e_v);
                band[j] = std::min(kMxMaxBands - 1, std::max(0, (e_top - e_v) / kMxBandBits));
                n_bands = std::max(n_bands, band[j] + 1);
            }
        }
        if (n_bands > 1) {
            std::vector<nps_row_desc> copy(d->m);
            for (int b = 0; b < n_bands; ++b) {
                nps_scoredef::MxBand mb;
                bool any = b == 0;
                for (uint64_t j = 0; j < d->m; ++j) {
                    copy[j] = data[j];
                    if (band[j] != b && std::isfinite(data[j].beta)) copy[j].beta = 0.0;
                    if (band[j] == b && std::isfinite(data[j].beta) && data[j].beta != 0.0) {
                        const double ie = std::isfinite(data[j].eaf) ? std::max(2.0, 2.0 * std::fabs(data[j].eaf)) : 2.0;
                        mb.bound = std::max(mb.bound, std::fabs(data[j].beta) * (4.0 + ie));
                        any = true;
                    }
                }
                if (!any) continue;  // an empty band costs no pass
                HIP_TRY(upload_desc(mb.d_desc, copy.data(), d->m));
                d->mx_bands.push_back(std::move(mb));
            }
        }
    }
    *out = owner.release();
    return NPS_OK;
}

extern "C" uint64_t nps_scoredef_n_present(const nps_scoredef *d) { return d ? d->m : 0; }

extern "C" void nps_scoredef_destroy(nps_scoredef *d) { delete d; }

// ------------------------------------------------------------------------------------------
// resident scoring.  Two-pass mode: per block of rows, tally -> params -> accumulate.
#ifdef NPS_DIAGNOSTICS
// run-time switches exist in diagnostics builds only (tools/mkexp.sh -DNPS_DIAGNOSTICS): the release
// library reads no environment variable on its launch path
static uint64_t env_u64(const char *name, uint64_t dflt) {
    const char *s = getenv(name);
    if (!s || !*s) return dflt;
    char *end = nullptr;
    unsigned long long v = strtoull(s, &end, 10);
    return end && *end == 0 ? (uint64_t)v : dflt;
}
#else
static inline uint64_t env_u64(const char *, uint64_t dflt) { return dflt; }
#endif

// stats of the last resident run stay on the device until somebody asks for them
static int materialize_resident_stats(nps_ctx *c) {
    if (!c->res_pending) return NPS_OK;
    std::vector<nps_locus_stat> dev(c->res_m);
    if (c->res_m) {
        HIP_TRY(hipMemcpyAsync(dev.data(), c->d_rstats.get(), sizeof(nps_locus_stat) * c->res_m,
                               hipMemcpyDeviceToHost, c->stream.get()));
        HIP_TRY(hipStreamSynchronize(c->stream.get()));
    }
    size_t h = 0;
    for (size_t j = 0; j < c->res_index.size(); ++j) {
        if (c->res_index[j] < 0) {
            c->ready.push_back(c->res_host_stats[h++]);
            continue;
        }
        c->ready.push_back(dev[(size_t)c->res_index[j]]);
    }
    c->res_pending = false;
    c->res_index.clear();
    c->res_host_stats.clear();
    return NPS_OK;
}

// NPS_FMT_GT2X runs of a definition with special rows (mx_special): the fixed-point pass scored them at beta = eaf = 0 --
// their tallies, statistics and decisions included, a product 0 x 0 is 0, and where it is NaN (an imputed NaN dosage) the
// reference's product is NaN for any beta too.  Here the same rows come out of the strip layout into the row layout, a
// batch at a time, and the two-pass row kernels add dosage x beta in IEEE double into the partial sums, with the
// decisions of their own tallies of the same codes (nloci is counted once: by the fixed-point pass).
static uint64_t mx_special_batch(const nps_ctx *c, uint64_t k) {
    const uint64_t row_bytes = (c->n_words + c->stride_words) * 4;
    const uint64_t cap = std::min<uint64_t>(std::max<uint64_t>(4, (64ull << 20) / row_bytes / 4 * 4), 65532ull * 4);
    return std::min(cap, (k + 3) / 4 * 4);
}

static int mx_special_buffers(nps_ctx *c, const nps_scoredef *def) {
    const uint64_t B = mx_special_batch(c, def->special.size());
    HIP_TRY(c->d_sp_plain.ensure(B * c->n_words, c->stream.get()));
    HIP_TRY(c->d_sp_group.ensure(B * c->stride_words, c->stream.get()));
    HIP_TRY(c->d_sp_tally.ensure(B, c->stream.get()));
    HIP_TRY(c->d_sp_lut.ensure(4 * B, c->stream.get()));
    return NPS_OK;
}

static int mx_special_pass(nps_ctx *c, const nps_cohort *co, uint64_t cohort_row0, const nps_scoredef *def,
                           unsigned long long *scratch_nloci) {
    const uint64_t K = def->special.size(), B = mx_special_batch(c, K);
    int rc = ensure_all_chunks(c);
    if (rc) return rc;
    ProfScope ps(c, P_ACCUM);
    // (more than one batch: tests/test_gpu_seams.py seam_special_rows_in_two_batches)
    for (uint64_t b0 = 0; b0 < K; b0 += B) {
        const uint64_t k = std::min(B, K - b0), k_pad = (k + 3) / 4 * 4;
        for (uint64_t j = b0; j < b0 + k;) {  // one launch per run of consecutive rows
            uint64_t e = j + 1;
            while (e < b0 + k && def->special[e] == def->special[e - 1] + 1) ++e;
            HIP_TRY(launch_gt2x_to_rows(c->stream.get(), co->d_data.get(), c->n, co->n_rows, cohort_row0 + def->special[j], e - j,
                                        c->d_sp_plain.get() + (j - b0) * c->n_words, c->n_words));
            j = e;
        }
        HIP_TRY(launch_interleave_rows(c->stream.get(), c->d_sp_plain.get(), c->n_words, k, c->n, nullptr, c->d_sp_group.get(),
                                       c->stride_words));
        HIP_TRY(launch_tally_packed(c->stream.get(), c->d_sp_group.get(), c->stride_words, c->n, k, c->d_sp_tally.get()));
        HIP_TRY(launch_row_params(c->stream.get(), c->d_sp_tally.get(), def->d_special.get() + b0, k, k_pad, c->n, dev_params(c->params),
                                  c->d_sp_lut.get(), nullptr, scratch_nloci));
        AccumGeom g = c->geom;
        g.groups_per_chunk = std::max<uint32_t>(1, (uint32_t)((k_pad / 4 + g.n_chunks - 1) / g.n_chunks));
        HIP_TRY(launch_accumulate(c->stream.get(), c->d_sp_group.get(), c->stride_words, k, c->d_sp_lut.get(), g, c->d_part.get()));
    }
    return NPS_OK;
}

// ---- nps_score_cohort_def and its three formats.  From the first launch that changes the context's sums an error leaves
// queued work behind: the context is marked broken.
struct RunGuard {
    nps_ctx *c;
    bool armed = false, ok = false;  // armed: a launch that changes the context's sums is queued
    ~RunGuard() { if (armed && !ok) c->broken = true; }
};

// the fused kernels' tally words must be zero on entry; their epilogue (fold_kernel) leaves them so
static int tally_ready(nps_ctx *c) {
    if (!c->rtally_clean)
        HIP_TRY(hipMemsetAsync(c->d_rtally.get(), 0, sizeof(unsigned long long) * c->d_rtally.cap(), c->stream.get()));
    c->rtally_clean = false;
    return NPS_OK;
}

static int fused_epilogue(nps_ctx *c, const FusedPlan &plan, uint64_t n_tally) {
    ProfScope ps(c, P_REDUCE);
    HIP_TRY(launch_fold(c->stream.get(), c->d_part_fused.get(), plan.Q, plan.part_team_stride, c->n, c->d_part.get(),
                        c->chunks_used == 0 ? 1 : 0, c->d_rtally.get(), n_tally, c->d_timeout.get(), c->d_nloci.get() + 1));
    c->chunks_used = std::max(c->chunks_used, 1u);
    c->rtally_clean = true;  // all words were zero before the run, [0, m_pad) are zero again
    return NPS_OK;
}

// The single-read kernel of the row and the DS layouts, and its epilogue.  *ran = false with NPS_OK: the runtime refused the
// cooperative grid (it would not be fully resident), nothing ran, and the caller scores the run in two reads -- only where
// that is allowed (NPS_MODE_AUTO; never NPS_FMT_DS16), everything else fails.
template <class Launch>
static int single_read(nps_ctx *c, RunGuard &guard, const FusedPlan &plan, uint64_t n_tally, const char *what,
                       bool may_fall_back, Launch launch, bool *ran) {
    *ran = false;
    int rc = tally_ready(c);
    if (rc) return rc;
    hipError_t fe;
    {
        ProfScope ps(c, P_FUSED);
        fe = launch();
    }
    if (fe == hipSuccess) {
        guard.armed = true;
        *ran = true;
        return fused_epilogue(c, plan, n_tally);
    }
    (void)hipGetLastError();
    c->rtally_clean = true;  // (zeroed above, untouched)
    if (!may_fall_back || fe != hipErrorCooperativeLaunchTooLarge)
        return fail(NPS_E_HIP, "%s kernel launch failed: %s", what, hipGetErrorString(fe));
    return NPS_OK;
}

// buffers of a strip run (a failed allocation leaves the context usable: nothing has been queued yet)
static int mx_run_buffers(nps_ctx *c, const nps_cohort *co, const nps_scoredef *def, uint64_t m_pad, MxRouted *mx) {
    const MxPlan &mxp = mx->plan;
    bool grew = false;
    HIP_TRY(c->d_mx_cpart.ensure(mxp.cpart_floats, c->stream.get()));
    HIP_TRY(c->d_mx_const.ensure(8 + 2ull * mxp.Q, c->stream.get(), &grew));
    if (grew) HIP_TRY(hipMemsetAsync(c->d_mx_const.get(), 0, sizeof(double) * c->d_mx_const.cap(), c->stream.get()));
    if (mx->route == MxRoute::InPassKeep) {  // (the cohort's kept tallies: allocated once, by whoever keeps them first)
        nps_cohort *mco = const_cast<nps_cohort *>(co);
        std::lock_guard<std::mutex> lk(mco->tally_mutex);
        if (mx_tallies_alloc(mco) != hipSuccess) {
            (void)hipGetLastError();
            mx->route = MxRoute::InPass;  // (no room: the pass runs as it always did)
        }
    }
    if (!def->special.empty()) {
        int rc = mx_special_buffers(c, def);
        if (rc) return rc;
    }
    if (mxp.given) {
        HIP_TRY(c->d_mx_ops.ensure(m_pad, c->stream.get()));
        HIP_TRY(c->d_mx_cblk.ensure(m_pad / 128, c->stream.get()));
    }
    grew = false;
    HIP_TRY(c->d_mx_tally1.ensure((uint64_t)((mxp.P + 15) / 16) * m_pad, c->stream.get(), &grew));
    if (grew)
        HIP_TRY(hipMemsetAsync(c->d_mx_tally1.get(), 0, sizeof(unsigned long long) * c->d_mx_tally1.cap(), c->stream.get()));
    return NPS_OK;
}

// NPS_FMT_GT2X: one pass per magnitude band of the definition (normally one) on the route mx_route chose
// (set: a subset run -- route GivenTallied, its tally pass counted under the set's mask, the decisions with N = kept samples)
static int score_run_mx(nps_ctx *c, RunGuard &guard, const nps_cohort *co, uint64_t cohort_row0, const nps_scoredef *def,
                        const MxRouted &mx, const nps_sampleset *set) {
    const MxPlan &mxp = mx.plan;
    const MxRoute route = mx.route;
    const size_t n_bands = std::max<size_t>(1, def->mx_bands.size());  // (no bands: the definition is its one band)
    unsigned long long *scratch_nloci = reinterpret_cast<unsigned long long *>(c->d_mx_const.get());  // (the 8 scratch doubles)
    MxRun r;
    r.d_units = co->d_data.get();
    r.n_sb_cohort = gt2x_superblocks(co->n_rows);
    r.sb0 = cohort_row0 >> 7;
    r.n_samples = c->n;
    r.n_decide = set ? set->n_kept : c->n;
    r.n_rows = def->m;
    r.prm = dev_params(c->params);
    r.t_maxmis = maxmis_threshold(r.n_decide, c->params.max_missing_rate);
    r.d_tally = c->d_rtally.get();
    r.d_const_sum = c->d_mx_const.get() + 8;
    r.d_cpart = c->d_mx_cpart.get();
    r.d_timeout = c->d_timeout.get();
    r.d_pre = c->d_rlut.get();
    r.d_tally1 = c->d_mx_tally1.get();
    r.d_tally_given = route == MxRoute::GivenKept ? co->d_mx_row_tally.get() + cohort_row0 : c->d_rtally.get();
    r.d_ops = c->d_mx_ops.get();
    r.d_const_part = c->d_mx_cblk.get();
    r.d_done = c->d_timeout.get() + 17;
    r.d_part0 = c->d_part.get();
    r.d_status = c->d_nloci.get() + 1;
    for (size_t b = 0; b < n_bands; ++b) {  // band 0 counts nloci and writes the statistics
        const bool banded = !def->mx_bands.empty();
        const double bound = banded ? def->mx_bands[b].bound : def->mx_bound;
        r.d_desc = banded ? def->mx_bands[b].d_desc.get() : def->d_mx_desc.get() ? def->d_mx_desc.get() : def->d_desc.get();
        // fixed-point scale: every weight of the band below 2^56 (fourteen hexadecimal digits)
        r.F = 56;
        if (bound > 0.0) {
            int e2 = 0;
            (void)std::frexp(bound, &e2);  // bound < 2^e2
            r.F = std::min(1000, std::max(-1000, 56 - e2));
        }
        r.d_stats = b == 0 ? c->d_rstats.get() : nullptr;
        r.d_nloci = b == 0 ? c->d_nloci.get() : scratch_nloci;
        r.overwrite = c->chunks_used == 0 ? 1 : 0;
        const bool keep = route == MxRoute::InPassKeep && b == 0;
        r.d_keep = keep ? co->d_mx_row_tally.get() : nullptr;
        r.n_keep = keep ? (uint64_t)mxp.n_sb * 128 : 0;
        int rc = tally_ready(c);
        if (rc) return rc;
        if (route == MxRoute::GivenTallied) {
            ProfScope ps(c, P_TALLY);
            if (set)
                HIP_TRY(launch_mx_tally_masked(c->stream.get(), mxp, r.d_units, r.n_sb_cohort, r.sb0, set->d_unit.get(),
                                               c->d_rtally.get()));
            else
                HIP_TRY(launch_mx_tally(c->stream.get(), mxp, r.d_units, r.n_sb_cohort, r.sb0, c->d_rtally.get()));
        }
        hipError_t fe;
        {
            ProfScope ps(c, mxp.given ? P_ACCUM : P_FUSED);
            fe = mxp.given ? launch_mx_given(c->stream.get(), mxp, r) : launch_fused_mx(c->stream.get(), mxp, r);
        }
        if (fe != hipSuccess) {
            (void)hipGetLastError();  // the runtime refused the cooperative grid: nothing ran
            c->rtally_clean = route != MxRoute::GivenTallied;
            return fail(NPS_E_HIP, "NPS_FMT_GT2X kernel launch failed: %s", hipGetErrorString(fe));
        }
        guard.armed = true;
        {
            ProfScope ps(c, P_REDUCE);
            HIP_TRY(launch_mx_fold(c->stream.get(), mxp, r));
            HIP_TRY(hipMemsetAsync(r.d_const_sum, 0, sizeof(double) * 2 * mxp.Q, c->stream.get()));
        }
        c->chunks_used = std::max(c->chunks_used, 1u);
        c->rtally_clean = true;
    }
    if (!def->special.empty()) {
        int rc = mx_special_pass(c, co, cohort_row0, def, scratch_nloci);
        if (rc) return rc;
    }
    if (route == MxRoute::InPassKeep) {
        // the kept tallies are published only once they ARE in device memory (another context may score this cohort
        // from another thread and stream): one wait, on the cohort's first pass only
        // (a superblock that was valid before -- rows uploaded, then others rewritten by the generator -- has received the
        //  same words again: a reader on another thread sees complete words at every moment)
        HIP_TRY(hipStreamSynchronize(c->stream.get()));
        nps_cohort *mco = const_cast<nps_cohort *>(co);
        std::lock_guard<std::mutex> lk(mco->tally_mutex);
        mx_tallies_mark(mco, 0, gt2x_superblocks(co->n_rows), true);
        mco->mx_tally_asked.store(true, std::memory_order_release);
    }
    return NPS_OK;
}

// NPS_FMT_DS32 / NPS_FMT_DS16: the single-read kernel (plan.ok), else -- float32 rows only -- tally, params, accumulate
// (set: a subset run -- always the three launches, the tally counted under the set's mask and the decisions with N = kept
// samples; the accumulation is the cohort's)
static int score_run_ds(nps_ctx *c, RunGuard &guard, const nps_cohort *co, uint64_t cohort_row0, const nps_scoredef *def,
                        int mode, const FusedPlan &plan, uint64_t n_tally, const nps_sampleset *set) {
    const uint64_t m = def->m;
    const uint64_t n_decide = set ? set->n_kept : c->n;
    const bool is_ds16 = co->format == NPS_FMT_DS16;
    const uint64_t stride_f = co->stride_bytes / 4;  // (NPS_FMT_DS32 only below the fused branch)
    const float *ds = (const float *)((const char *)co->d_data.get() + cohort_row0 * co->stride_bytes);
    if (plan.ok && c->n && !set) {
        bool ran = false;
        int rc = single_read(c, guard, plan, n_tally, "fused DS", mode == NPS_MODE_AUTO && !is_ds16, [&]() {
            return launch_ds_fused(c->stream.get(), plan, ds, co->stride_bytes, is_ds16 ? 2 : 4, c->n, m, def->d_desc.get(),
                                   dev_params(c->params), maxmis_threshold(c->n, c->params.max_missing_rate), c->d_rtally.get(),
                                   c->d_rstats.get(), c->d_nloci.get(), c->d_part_fused.get(), c->d_timeout.get());
        }, &ran);
        if (rc || ran) return rc;
    }
    if (is_ds16) return fail(NPS_E_UNSUPPORTED, "NPS_FMT_DS16 cohorts are scored by the single-read kernel only");
    // launches of >= 2048 rows keep every CU busy in both kernels (one workgroup per row in the
    // tally; samples x row chunks in the accumulation)
    uint64_t block_rows = env_u64("NPS_BLOCK_ROWS", 0);
    if (block_rows == 0) block_rows = std::max<uint64_t>(2048, (256ull << 20) / co->stride_bytes);
    int rc = ensure_all_chunks(c);
    if (rc) return rc;
    guard.armed = true;
    // (more than one block: tests/test_gpu_seams.py seam_ds32_two_pass_blocks)
    for (uint64_t r0 = 0; r0 < m; r0 += block_rows) {
        const uint64_t k = std::min(block_rows, m - r0);
        {
            ProfScope ps(c, P_TALLY);
            HIP_TRY(launch_ds_tally(c->stream.get(), ds + r0 * stride_f, stride_f, c->n, def->d_desc.get() + r0, k,
                                    set ? set->d_bits.get() : nullptr, c->d_rds_tally.get() + r0));
        }
        {
            ProfScope ps(c, P_PARAMS);
            HIP_TRY(launch_ds_params(c->stream.get(), c->d_rds_tally.get() + r0, def->d_desc.get() + r0, k, n_decide,
                                     dev_params(c->params), c->d_rds_rowp.get() + r0, c->d_rstats.get() + r0,
                                     c->d_nloci.get()));
        }
        {
            ProfScope ps(c, P_ACCUM);
            HIP_TRY(launch_ds_accumulate(c->stream.get(), ds + r0 * stride_f, stride_f, c->n,
                                         c->d_rds_rowp.get() + r0, k, c->d_part.get(), c->n_chunks,
                                         c->geom.part_chunk_stride));
        }
    }
    return NPS_OK;
}

// NPS_FMT_GT2: the single-read kernel (plan.ok), else per block of rows tally, params, accumulate
static int score_run_gt2(nps_ctx *c, RunGuard &guard, const nps_cohort *co, uint64_t cohort_row0, const nps_scoredef *def,
                         int mode, const FusedPlan &plan, uint64_t n_tally) {
    const uint64_t m = def->m;
    const uint64_t stride_words = co->stride_bytes / 4;
    const uint32_t *codes = (const uint32_t *)co->d_data.get() + (cohort_row0 >> 2) * stride_words * 4;
    const nps_row_desc *d_desc = def->d_desc.get();
    const int parity = co->optimized ? 1 : 0;  // the kernels undo the parity layout for the tally
    if (plan.ok && c->n) {
        bool ran = false;
        int rc = single_read(c, guard, plan, n_tally, "fused", mode == NPS_MODE_AUTO, [&]() {
            return launch_fused(c->stream.get(), plan, codes, stride_words, c->n, m, d_desc, dev_params(c->params), c->d_rtally.get(),
                                c->d_rstats.get(), c->d_nloci.get(), c->d_part_fused.get(), c->d_timeout.get(), parity);
        }, &ran);
#ifdef NPS_DIAGNOSTICS
        if (rc == NPS_OK && ran && getenv("NPS_TELEMETRY")) {  // diagnostics of the control wave (cycles, summed)
            unsigned long long t[8] = {0};
            (void)hipStreamSynchronize(c->stream.get());
            (void)hipMemcpy(t, (char *)c->d_timeout.get() + 16, sizeof t, hipMemcpyDeviceToHost);
            (void)hipMemset((char *)c->d_timeout.get() + 16, 0, sizeof t);
            const double wg = (double)plan.P * plan.Q, st = t[4] ? (double)t[4] : 1.0;
            fprintf(stderr, "[nps] fused P=%u Q=%u T=%u: per step per WG: spins %.2f, poll wait "
                    "%.0f cyc, control chain %.0f cyc, barrier wait %.0f cyc (steps/WG %.0f)\n",
                    plan.P, plan.Q, plan.threads, t[0] / st, t[1] / st, t[2] / st, t[3] / st, st / wg);
        }
#endif
        if (rc || ran) return rc;
    }
    // rows per tally/accumulate pair; default ~96 MB so the second read can hit the 256 MB
    // Infinity Cache
    uint64_t block_rows = env_u64("NPS_BLOCK_ROWS", 0);
    if (block_rows == 0) block_rows = std::max<uint64_t>(64, (96ull << 20) / co->stride_bytes);
    block_rows = (block_rows + 15) / 16 * 16;
    int rc = ensure_all_chunks(c);
    if (rc) return rc;
    guard.armed = true;
    c->rtally_clean = false;  // the two-pass tally kernel leaves its counts in d_rtally
    // (more than one block: tests/test_gpu_seams.py seam_tall_row_two_pass_blocks)
    for (uint64_t r0 = 0; r0 < m; r0 += block_rows) {
        const uint64_t k = std::min(block_rows, m - r0);
        const uint64_t k_pad = (k + 3) / 4 * 4;  // only the last block can be ragged
        {
            ProfScope ps(c, P_TALLY);
            HIP_TRY(launch_tally_packed(c->stream.get(), codes + (r0 >> 2) * stride_words * 4, stride_words,
                                        c->n, k, c->d_rtally.get() + r0, parity));
        }
        {
            ProfScope ps(c, P_PARAMS);
            HIP_TRY(launch_row_params(c->stream.get(), c->d_rtally.get() + r0, d_desc + r0, k, k_pad, c->n,
                                      dev_params(c->params), c->d_rlut.get() + r0 * 4, c->d_rstats.get() + r0,
                                      c->d_nloci.get()));
        }
        if (c->n) {
            AccumGeom g = c->geom;
            const uint32_t groups = (uint32_t)(k_pad / 4);
            g.groups_per_chunk = std::max(1u, (groups + g.n_chunks - 1) / g.n_chunks);
            ProfScope ps(c, P_ACCUM);
            HIP_TRY(launch_accumulate(c->stream.get(), codes + (r0 >> 2) * stride_words * 4, stride_words, k,
                                      c->d_rlut.get() + r0 * 4, g, c->d_part.get(), parity));
        }
    }
    return NPS_OK;
}

// the single-read plan of a row-layout or DS run (cached on the context), and what refuses it before anything changes
static int fused_plan_for_run(nps_ctx *c, const nps_cohort *co, uint64_t m, int mode, FusedPlan *plan) {
    const bool is_ds16 = co->format == NPS_FMT_DS16, is_ds = co->format == NPS_FMT_DS32 || is_ds16;
    if (c->plan_valid && c->plan_fmt == co->format && c->plan_m == m) {
        *plan = c->plan_cache;
    } else {
        const int want = (int)env_u64("NPS_FUSED_THREADS", 0), max_q = (int)env_u64("NPS_FUSED_MAXQ", 0);
        if (is_ds)
            HIP_TRY(ds_fused_plan(c->device, c->n, m, want, max_q, plan, is_ds16 ? 2 : 4));
        else
            HIP_TRY(fused_plan(c->device, c->n, m, want, max_q, plan));
        c->plan_cache = *plan;
        c->plan_fmt = co->format;
        c->plan_m = m;
        c->plan_valid = true;
    }
    if (env_u64("NPS_DISABLE_FUSED", 0) == 1 && mode == NPS_MODE_AUTO) plan->ok = false;
    if (is_ds && co->ds_bad_rows) {  // a dosage outside [0, 2] somewhere in the cohort: the two-pass kernels take any value
        if (mode == NPS_MODE_FUSED)
            return fail(NPS_E_INVAL, "%llu row(s) of the cohort hold FORMAT/DS values outside [0, 2]: the single-read DS "
                        "kernel hands dosage sums over in fixed point and needs that range (NPS_MODE_AUTO / "
                        "NPS_MODE_TWOPASS score such a cohort in two reads)", (unsigned long long)co->ds_bad_rows);
        plan->ok = false;
    }
    if (!plan->ok && (mode == NPS_MODE_FUSED || is_ds16))
        return fail(NPS_E_UNSUPPORTED, "shape (%llu samples, %llu rows) does not fit the fused "
                    "persistent grid%s", (unsigned long long)c->n, (unsigned long long)m,
                    is_ds16 ? " (NPS_FMT_DS16 has no two-read kernels: use NPS_FMT_DS32)" : "");
    return NPS_OK;
}

// Everything that can be refused is checked BEFORE the context changes: a call that returns an error
// from its validation leaves the context exactly as it was, so it can be repeated (e.g. in another
// mode).  The rows without genotype data are applied, and the run is registered for nps_flush, only
// once all launches have been queued; a failure between the first and the last launch marks the
// context broken (NPS_E_STATE until nps_reset).
// set: nps_score_cohort_def_subset (mode NPS_MODE_TWOPASS: the routes that count the tallies in a pass of their own), else null
static int score_cohort_def(nps_ctx *c, const nps_cohort *co, uint64_t cohort_row0, const nps_scoredef *def, int mode,
                            const nps_sampleset *set) {
    int rc = check_usable(c);
    if (rc) return rc;
    if (!co || !def) return fail(NPS_E_INVAL, "cohort or scoredef is NULL");
    if (co->device != c->device || def->device != c->device)
        return fail(NPS_E_INVAL, "cohort / scoredef / context on different devices");
    if (co->n_samples != c->n)
        return fail(NPS_E_INVAL, "cohort has %llu samples, context %llu",
                    (unsigned long long)co->n_samples, (unsigned long long)c->n);
    if (mode != NPS_MODE_AUTO && mode != NPS_MODE_TWOPASS && mode != NPS_MODE_FUSED)
        return fail(NPS_E_INVAL, "bad mode %d", mode);
    const uint64_t m = def->m;
    rc = check_range(co, cohort_row0, m);
    if (rc) return rc;
    if (co->format == NPS_FMT_GT2M)
        return fail(NPS_E_UNSUPPORTED, "NPS_FMT_GT2M cohorts are scored with nps_score_cohort_multi");
    rc = cohort_quiesce(co);  // rows pushed into the cohort (nps_cohort_push_*) are complete
    if (rc) return rc;
    const bool is_ds16 = co->format == NPS_FMT_DS16;
    const bool is_ds = co->format == NPS_FMT_DS32 || is_ds16;
    const bool is_mx = co->format == NPS_FMT_GT2X;
    if (is_ds16 && mode == NPS_MODE_TWOPASS)
        return fail(NPS_E_UNSUPPORTED, "NPS_FMT_DS16 cohorts are scored by the single-read kernel only");
    if (is_mx && (cohort_row0 & 127))
        return fail(NPS_E_INVAL, "cohort_row0 must be a multiple of 128 for NPS_FMT_GT2X cohorts");
    if (!is_ds && (cohort_row0 & 3))
        return fail(NPS_E_INVAL, "cohort_row0 must be a multiple of 4 (rows are stored in groups of 4)");
    HIP_TRY(hipSetDevice(c->device));
    MxRouted mx;  // NPS_FMT_GT2X: which kernel scores the run, where its row tallies come from, and the plan (nps_mx_route.h)
    if (is_mx && m && c->n) {
        MxRouteIn in;
        in.mode = mode;
        HIP_TRY(mx_cus(c->device, &in.cus));
        in.n_samples = c->n;
        in.m = m;
        in.n_rows_cohort = co->n_rows;
        in.cohort_row0 = cohort_row0;
        in.run_tallies_valid = mx_tallies_valid(co, cohort_row0 >> 7, (m + 127) / 128);
        in.tallies_asked = co->mx_tally_asked.load(std::memory_order_acquire);
        in.expect_passes = co->expect_passes.load(std::memory_order_relaxed);
        mx = mx_route(in);
        if (!mx.ok)
            return fail(NPS_E_UNSUPPORTED, "shape (%llu samples, %llu rows) is beyond the NPS_FMT_GT2X kernels (2^27 samples)",
                        (unsigned long long)c->n, (unsigned long long)m);
        if (mx.refused_fused)
            return fail(NPS_E_UNSUPPORTED, "shape (%llu samples, %llu rows) does not fit the persistent grid of the "
                        "single-read NPS_FMT_GT2X kernel (one 2048-sample strip per compute unit); NPS_MODE_AUTO "
                        "scores it in two reads", (unsigned long long)c->n, (unsigned long long)m);
        if (mx.count_cohort_first) {
            nps_cohort *mco = const_cast<nps_cohort *>(co);
            std::lock_guard<std::mutex> lk(mco->tally_mutex);
            rc = mx_keep_tallies_locked(mco);  // (counts what is not valid yet: nothing, if another thread was first)
            if (rc) return rc;
            HIP_TRY(hipSetDevice(c->device));
        }
#ifdef NPS_DIAGNOSTICS
        if (getenv("NPS_MXG_Q")) HIP_TRY(mx_plan(c->device, c->n, m, mx.plan.given, &mx.plan));  // (mx_plan's override)
#endif
    }
    FusedPlan plan;
    if (!is_mx && mode != NPS_MODE_TWOPASS && m && c->n) {
        rc = fused_plan_for_run(c, co, m, mode, &plan);
        if (rc) return rc;
    }

    rc = run_batch(c);  // keep push order: finish whatever was streamed before
    if (rc) return rc;
    rc = materialize_resident_stats(c);
    if (rc) return rc;

    // the run is registered only after its launches are queued (commit below)
    auto commit = [&]() {
        c->res_host_stats.clear();
        c->res_host_stats.reserve(def->host_rows.size());
        for (const nps_row_desc &r : def->host_rows) {  // host decided; nimpress.nim:526-558
            nps_locus_stat st;
            host_locus_row(c, r.kind, r.ref_is_effect, r.beta, r.eaf, &st);
            c->res_host_stats.push_back(st);
        }
        c->res_index = def->data_index;
        c->res_m = m;
        c->res_pending = true;
    };
    if (m == 0) {
        commit();
        return NPS_OK;
    }

    // buffers (a failed allocation leaves the context usable: nothing has been queued yet)
    const uint64_t m_pad = is_mx ? (m + 127) / 128 * 128 : (m + 15) / 16 * 16;
    const bool fused = plan.ok && c->n;
    // (the single-read DS kernel keeps a PAIR of tally words per row)
    const uint64_t n_tally = is_ds && fused ? 2 * m_pad : m_pad;
    bool grew = false;
    const hipError_t ge = c->d_rtally.ensure(n_tally, c->stream.get(), &grew);
    if (grew) c->rtally_clean = false;  // (also where the allocation then failed: the old words are gone)
    HIP_TRY(ge);
    HIP_TRY(c->d_rlut.ensure(4 * n_tally, c->stream.get()));
    HIP_TRY(c->d_rstats.ensure(n_tally, c->stream.get()));
    if (is_mx && c->n) {
        rc = mx_run_buffers(c, co, def, m_pad, &mx);
        if (rc) return rc;
    }
    if (fused) HIP_TRY(c->d_part_fused.ensure((uint64_t)plan.Q * plan.part_team_stride, c->stream.get()));
    if (is_ds) {
        HIP_TRY(c->d_rds_tally.ensure(m_pad, c->stream.get()));
        HIP_TRY(c->d_rds_rowp.ensure(m_pad, c->stream.get()));
    }

    // ---- launches
    RunGuard guard{c};
    if (is_mx)
        rc = c->n ? score_run_mx(c, guard, co, cohort_row0, def, mx, set) : NPS_OK;
    else if (is_ds)
        rc = score_run_ds(c, guard, co, cohort_row0, def, mode, plan, n_tally, set);
    else
        rc = score_run_gt2(c, guard, co, cohort_row0, def, mode, plan, n_tally);
    if (rc) return rc;
    commit();
    guard.ok = true;
    return NPS_OK;
}

extern "C" int nps_score_cohort_def(nps_ctx *c, const nps_cohort *co, uint64_t cohort_row0,
                                    const nps_scoredef *def, int mode) {
    return score_cohort_def(c, co, cohort_row0, def, mode, nullptr);
}

// ------------------------------------------------------------------------------------------
// a subset of a resident cohort's samples (the kernels: nps_subset.hip)
extern "C" int nps_sampleset_create(nps_sampleset **out, int device, uint64_t n_samples, const uint8_t *keep) {
    if (!out) return fail(NPS_E_INVAL, "out is NULL");
    *out = nullptr;
    if (!keep) return fail(NPS_E_INVAL, "keep is NULL");
    if (n_samples == 0) return fail(NPS_E_INVAL, "a sample set of no samples");
    if (n_samples > 0x7fffffffull) return fail(NPS_E_UNSUPPORTED, "n_samples %llu exceeds 2^31-1", (unsigned long long)n_samples);
    const SubsetMask m = subset_mask(keep, n_samples);
    if (m.n_kept == 0) return fail(NPS_E_INVAL, "the sample set keeps none of its %llu samples", (unsigned long long)n_samples);
    int rc = select_device(device);
    if (rc) return rc;
    std::unique_ptr<nps_sampleset> owner(new (std::nothrow) nps_sampleset);
    nps_sampleset *s = owner.get();
    if (!s) return fail(NPS_E_NOMEM, "out of host memory");
    s->device = device;
    s->n_samples = n_samples;
    s->n_kept = m.n_kept;
    HIP_TRY(s->d_bits.alloc(m.bits.size()));
    HIP_TRY(s->d_unit.alloc(m.unit.size()));
    HIP_TRY(s->d_prefix.alloc(m.prefix.size()));
    HIP_TRY(hipMemcpy(s->d_bits.get(), m.bits.data(), sizeof(uint32_t) * m.bits.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->d_unit.get(), m.unit.data(), sizeof(uint64_t) * m.unit.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->d_prefix.get(), m.prefix.data(), sizeof(uint32_t) * m.prefix.size(), hipMemcpyHostToDevice));
    *out = owner.release();
    return NPS_OK;
}
extern "C" uint64_t nps_sampleset_n_samples(const nps_sampleset *s) { return s ? s->n_samples : 0; }
extern "C" uint64_t nps_sampleset_n_kept(const nps_sampleset *s) { return s ? s->n_kept : 0; }
extern "C" void nps_sampleset_destroy(nps_sampleset *s) { delete s; }

static const char *format_name(int format) {
    switch (format) {
    case NPS_FMT_GT2: return "NPS_FMT_GT2";
    case NPS_FMT_DS32: return "NPS_FMT_DS32";
    case NPS_FMT_GT2M: return "NPS_FMT_GT2M";
    case NPS_FMT_GT2X: return "NPS_FMT_GT2X";
    case NPS_FMT_DS16: return "NPS_FMT_DS16";
    default: return "unknown format";
    }
}

// Everything is refused before the context changes, as for nps_score_cohort_def.  The run takes the routes that count the
// rows' tallies in a pass of their own (NPS_MODE_TWOPASS) into the CONTEXT's tally buffer: the tallies a cohort keeps are
// whole-cohort tallies and are neither read nor written here.
extern "C" int nps_score_cohort_def_subset(nps_ctx *c, const nps_cohort *co, uint64_t cohort_row0, const nps_scoredef *def,
                                           const nps_sampleset *s) {
    int rc = check_usable(c);
    if (rc) return rc;
    if (!co || !def) return fail(NPS_E_INVAL, "cohort or scoredef is NULL");
    rc = check_sampleset(c, s);
    if (rc) return rc;
    if (s->n_samples != co->n_samples)
        return fail(NPS_E_INVAL, "sample set has %llu samples, cohort %llu", (unsigned long long)s->n_samples,
                    (unsigned long long)co->n_samples);
    if (co->format != NPS_FMT_GT2X && co->format != NPS_FMT_DS32)
        return fail(NPS_E_UNSUPPORTED, "a subset of the samples is scored on NPS_FMT_GT2X and NPS_FMT_DS32 cohorts; this one is %s",
                    format_name(co->format));
    if (co->format == NPS_FMT_GT2X && !def->special.empty()) {
        // (the IEEE pass of such rows, mx_special_pass, recounts them with whole-cohort tallies)
        uint64_t j = 0;
        while (j < def->n_desc && def->data_index[j] != (int64_t)def->special[0]) ++j;
        return fail(NPS_E_UNSUPPORTED, "row %llu has a non-finite or extreme beta or an infinite eaf: NPS_FMT_GT2X cohorts score "
                    "such rows in an IEEE pass of whole-cohort tallies, which a subset run cannot use", (unsigned long long)j);
    }
    return score_cohort_def(c, co, cohort_row0, def, NPS_MODE_TWOPASS, s);
}

extern "C" int nps_score_cohort(nps_ctx *c, const nps_cohort *co, uint64_t cohort_row0,
                                const nps_row_desc *rows, uint64_t n_desc, int mode) {
    if (!c || !co) return fail(NPS_E_INVAL, "ctx or cohort is NULL");
    nps_scoredef *def = nullptr;
    int rc = nps_scoredef_create(&def, c->device, rows, n_desc);
    if (rc) return rc;
    rc = nps_score_cohort_def(c, co, cohort_row0, def, mode);
    // the launches read def->d_desc: complete them before the temporary definition goes away
    if (rc == NPS_OK) {
        hipError_t e = hipStreamSynchronize(c->stream.get());
        if (e != hipSuccess) rc = fail(NPS_E_HIP, "resident scoring failed: %s", hipGetErrorString(e));
    }
    nps_scoredef_destroy(def);
    return rc;
}

// ------------------------------------------------------------------------------------------
// several score definitions in one pass over a NPS_FMT_GT2M cohort (nps_multi.hip), in two over a dosage cohort (nps_multi_ds.hip)
extern "C" int nps_cohort_convert(nps_cohort *dst, const nps_cohort *src) {
    if (!dst || !src) return fail(NPS_E_INVAL, "cohort is NULL");
    if ((dst->format != NPS_FMT_GT2M && dst->format != NPS_FMT_GT2X) || src->format != NPS_FMT_GT2)
        return fail(NPS_E_INVAL, "nps_cohort_convert goes from a NPS_FMT_GT2 to a NPS_FMT_GT2M or NPS_FMT_GT2X cohort");
    if (dst->device != src->device || dst->n_samples != src->n_samples || dst->n_rows != src->n_rows)
        return fail(NPS_E_INVAL, "source and destination differ in device, samples or rows");
    if (src->optimized)
        return fail(NPS_E_STATE, "the source cohort is in the nps_cohort_optimize layout; convert it before optimising");
    HIP_TRY(hipSetDevice(dst->device));
    { int qrc = cohort_quiesce(src); if (qrc) return qrc; }
    HIP_TRY(hipDeviceSynchronize());
    if (src->n_rows == 0 || src->n_samples == 0) return NPS_OK;
    if (dst->format == NPS_FMT_GT2X) {  // units and, from the same tiles, the tally words of every superblock
        if (dst->n_samples >= (1ull << 27)) return fail(NPS_E_UNSUPPORTED, "more than 2^27 samples");
        mx_tallies_rewrite(dst, 0, dst->n_rows);
        std::lock_guard<std::mutex> lk(dst->tally_mutex);
        const uint64_t n_sb = gt2x_superblocks(dst->n_rows);
        HIP_TRY(mx_tallies_alloc(dst));
        HIP_TRY(hipMemsetAsync(dst->d_mx_row_tally.get(), 0, sizeof(unsigned long long) * n_sb * 128, nullptr));
        HIP_TRY(launch_fill_gt2x_from_gt2(nullptr, (const uint32_t *)src->d_data.get(), src->stride_bytes / 4, src->n_samples,
                                          src->n_rows, dst->d_data.get(), dst->d_mx_row_tally.get()));
        HIP_TRY(hipDeviceSynchronize());
        mx_tallies_mark(dst, 0, n_sb, true);
        return NPS_OK;
    }
    // units and, from the same tiles, the whole-row tallies (tallyAlleles nimpress.nim:32-47)
    HIP_TRY(launch_convert_gt2m(nullptr, (const uint32_t *)src->d_data.get(), src->stride_bytes / 4, src->n_samples,
                                src->n_rows, dst->d_data.get(), dst->d_row_tally.get()));
    HIP_TRY(hipDeviceSynchronize());
    return NPS_OK;
}

extern "C" int nps_cohort_row_tallies(const nps_cohort *c, uint64_t row0, uint64_t nrows, uint64_t *nmissing_out,
                                      uint64_t *neffect_out) {
    int rc = check_range(c, row0, nrows);
    if (rc) return rc;
    const bool kept = c->format == NPS_FMT_GT2X && nps_cohort_rows_tallied(c, row0, nrows);
    if (c->format != NPS_FMT_GT2M && !kept)
        return fail(NPS_E_UNSUPPORTED, "row tallies are kept with NPS_FMT_GT2M cohorts, and with the superblocks of a "
                                       "NPS_FMT_GT2X cohort that were uploaded / converted or counted since they were last "
                                       "written (nps_cohort_rows_tallied tells; nps_cohort_keep_tallies counts the rest)");
    if (nrows == 0) return NPS_OK;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<unsigned long long> t(nrows);
    HIP_TRY(hipMemcpy(t.data(), (kept ? c->d_mx_row_tally.get() : c->d_row_tally.get()) + row0, sizeof(unsigned long long) * nrows,
                      hipMemcpyDeviceToHost));
    for (uint64_t j = 0; j < nrows; ++j) {
        if (nmissing_out) nmissing_out[j] = kept ? (t[j] >> 28) & 0xfffffffull : t[j] >> 32;
        if (neffect_out) neffect_out[j] = kept ? t[j] & 0xfffffffull : t[j] & 0xffffffffull;
    }
    return NPS_OK;
}

// Experiment B of the round-4 verdict: a NPS_FMT_GT2X cohort that carries its whole-row tallies (tallyAlleles,
// nimpress.nim:32-47, of every row over all samples), counted ONCE by mx_tally_kernel.  nps_score_cohort[_def] with
// NPS_MODE_AUTO then scores the cohort with the tallies given: one read of the matrix, no popcounts, no hand-over
// between the strips, an ordinary grid.  For many score files over one cohort (BASELINE configs[3]: tally once, score
// eight times).  Rows that are uploaded or converted bring their tallies along (the fill kernels count while they write: nothing is
// read here for them); the generator's rows do not.
// tally_mutex held: counts the superblocks that are not valid (nothing where all are: no read) and sets the mark
static int mx_keep_tallies_locked(nps_cohort *c) {
    const uint64_t n_sb = gt2x_superblocks(c->n_rows);
    if (c->n_samples >= (1ull << 27)) return fail(NPS_E_UNSUPPORTED, "more than 2^27 samples");
    HIP_TRY(hipSetDevice(c->device));
    if (!mx_tallies_all_valid(c)) {
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(mx_tallies_alloc(c));
        if (c->n_samples) {
            MxPlan mp;
            HIP_TRY(mx_plan(c->device, c->n_samples, c->n_rows, true, &mp));
            if (!mp.ok) return fail(NPS_E_UNSUPPORTED, "shape beyond the NPS_FMT_GT2X kernels");
            // every maximal range of superblocks without tallies: valid words are never touched (a context on another
            // thread may be scoring from them)
            for (uint64_t sb = 0; sb < n_sb;) {
                if (mx_tallies_valid(c, sb, 1)) {
                    ++sb;
                    continue;
                }
                uint64_t e = sb + 1;
                while (e < n_sb && !mx_tallies_valid(c, e, 1)) ++e;
                HIP_TRY(hipMemsetAsync(c->d_mx_row_tally.get() + sb * 128, 0, sizeof(unsigned long long) * (e - sb) * 128, nullptr));
                mp.n_sb = (uint32_t)(e - sb);
                HIP_TRY(launch_mx_tally(nullptr, mp, c->d_data.get(), n_sb, sb, c->d_mx_row_tally.get() + sb * 128));
                sb = e;
            }
            HIP_TRY(hipDeviceSynchronize());
        }
        mx_tallies_mark(c, 0, n_sb, true);
    }
    c->mx_tally_asked.store(true, std::memory_order_release);
    return NPS_OK;
}
extern "C" int nps_cohort_keep_tallies(nps_cohort *c) {
    if (!c) return fail(NPS_E_INVAL, "cohort is NULL");
    if (c->format != NPS_FMT_GT2X)
        return fail(NPS_E_UNSUPPORTED, "nps_cohort_keep_tallies is for NPS_FMT_GT2X cohorts (NPS_FMT_GT2M carries its tallies "
                                       "from the packer; the other layouts count while they read)");
    std::lock_guard<std::mutex> lk(c->tally_mutex);
    return mx_keep_tallies_locked(c);
}
extern "C" int nps_cohort_expect_passes(nps_cohort *c, uint32_t n_passes) {
    if (!c) return fail(NPS_E_INVAL, "cohort is NULL");
    c->expect_passes.store(n_passes, std::memory_order_relaxed);
    return NPS_OK;
}
extern "C" int nps_cohort_has_tallies(const nps_cohort *c) {
    if (!c) return 0;
    if (c->format == NPS_FMT_GT2M) return 1;
    if (c->format != NPS_FMT_GT2X || !mx_tallies_all_valid(c)) return 0;
    return c->n_rows || c->mx_tally_asked.load(std::memory_order_acquire) ? 1 : 0;  // (no rows: once asked for, as before)
}
extern "C" int nps_cohort_rows_tallied(const nps_cohort *c, uint64_t row0, uint64_t nrows) {
    if (!c || row0 > c->n_rows || nrows > c->n_rows - row0) return 0;
    if (c->format == NPS_FMT_GT2M) return 1;
    if (c->format != NPS_FMT_GT2X) return 0;
    if (nrows == 0) return nps_cohort_has_tallies(c);
    return mx_tallies_valid(c, row0 >> 7, ((row0 + nrows + 127) >> 7) - (row0 >> 7)) ? 1 : 0;
}

struct nps_multidef {
    int device = 0;
    int S = 0;
    uint64_t n_desc = 0;
    DevBuf<nps_row_desc> d_desc;     // [S][n_desc]
    DevBuf<int> d_F;                 // fixed-point exponent per score: weight * 2^F is an integer below 2^(8 ND - 9)
    int ND = 7;                      // base-256 digits per weight
    int no_scale = -1;               // first score whose weight bound is not finite: no fixed-point scale (NPS_FMT_GT2M refuses it)

    ~nps_multidef() {  // a pass that reads the definitions may still be queued
        (void)hipSetDevice(device);
        (void)hipDeviceSynchronize();
    }
};

extern "C" int nps_multidef_create_bits(nps_multidef **out, int device, const nps_row_desc *rows, int n_scores,
                                        uint64_t n_desc, int weight_bits) {
    if (!out) return fail(NPS_E_INVAL, "out is NULL");
    *out = nullptr;
    if (weight_bits != 0 && weight_bits != 41 && weight_bits != 49)
        return fail(NPS_E_INVAL, "weight_bits must be 41 or 49 (0 = default 49), not %d", weight_bits);
    const int ND = weight_bits == 41 ? 6 : 7;
    if (n_scores < 1 || n_scores > NPS_MULTI_MAX_SCORES)
        return fail(NPS_E_INVAL, "n_scores %d outside 1..%d", n_scores, NPS_MULTI_MAX_SCORES);
    if (n_desc && !rows) return fail(NPS_E_INVAL, "rows is NULL");
    if (n_desc > 0xfffffff0ull) return fail(NPS_E_UNSUPPORTED, "too many rows");
    int F[NPS_MULTI_MAX_SCORES];
    int no_scale = -1;
    for (int s = 0; s < n_scores; ++s) {
        double maxb = 0.0, maxe = 0.0, minb = HUGE_VAL;
        for (uint64_t j = 0; j < n_desc; ++j) {
            const nps_row_desc &r = rows[(uint64_t)s * n_desc + j];
            if (r.kind < NPS_ROW_PRESENT || r.kind > NPS_ROW_NOT_IN_SCORE)
                return fail(NPS_E_INVAL, "score %d row %llu: bad kind %d", s, (unsigned long long)j, r.kind);
            if (r.kind == NPS_ROW_NOT_IN_SCORE) continue;
            if (!std::isfinite(r.beta))
                return fail(NPS_E_UNSUPPORTED, "score %d row %llu: beta is not finite (use the single-score path)",
                            s, (unsigned long long)j);
            if (std::isinf(r.eaf))  // (its imputed products are +-inf: the kernels keep one NaN flag; a NaN eaf is scored)
                return fail(NPS_E_UNSUPPORTED, "score %d row %llu: eaf is infinite (use the single-score path)", s,
                            (unsigned long long)j);
            maxb = std::max(maxb, std::fabs(r.beta));
            if (r.beta != 0.0) minb = std::min(minb, std::fabs(r.beta));
            if (std::isfinite(r.eaf)) maxe = std::max(maxe, std::fabs(r.eaf));
        }
        // One fixed-point scale per score: a weight is rounded to 2^-(8 ND - 9) of the largest one (x 5 for the imputation
        // range), so a sample that carries only the score's SMALL-beta rows keeps 1e-6 relative only while
        // 2.5 max|beta| / min|beta| <= 1e-6 x 2^(8 ND - 9): 2^25 for seven digits, 2^17 for six.  Beyond that the
        // definition is refused here -- the single-score path (nps_scoredef_create + nps_score_cohort_def) scores such a
        // definition in magnitude bands -- instead of silently losing those samples.
        const double span_limit = std::ldexp(1.0, ND == 7 ? 25 : 17);
        if (maxb > 0.0 && maxb / minb > span_limit)
            return fail(NPS_E_UNSUPPORTED, "score %d: |beta| spans %.3g (%.3g .. %.3g), more than the 2^%d one %d-bit "
                        "fixed-point scale holds within 1e-6 relative; score this definition with the single-score path "
                        "(nps_scoredef_create / nps_score_cohort_def: magnitude bands), the others in one pass",
                        s, maxb / minb, minb, maxb, ND == 7 ? 25 : 17, 8 * ND - 7);
        // largest weight a row can have: |beta| * max(|imputed - 3|, |locus constant|)
        const double bound = maxb * (3.0 + std::max(2.0, 2.0 * maxe));
        // Finite betas whose bound overflows (|beta| = DBL_MAX) have no scale: frexp leaves e unspecified, and the weights
        // beta x 2^F would not be integers llrint can hold.  The dosage formats score such a definition in plain float64,
        // so it is not refused here but by nps_score_cohort_multi on a NPS_FMT_GT2M cohort.
        int e = 0;
        if (!std::isfinite(bound)) {
            if (no_scale < 0) no_scale = s;
        } else if (bound > 0.0) {
            (void)std::frexp(bound, &e);  // bound < 2^e
        }
        F[s] = 8 * ND - 9 - e;  // the kernel's coefficients (up to 160 x weight) stay below 2^(8 ND - 1)
    }
    int rc = select_device(device);
    if (rc) return rc;
    std::unique_ptr<nps_multidef> owner(new (std::nothrow) nps_multidef);
    nps_multidef *d = owner.get();
    if (!d) return fail(NPS_E_NOMEM, "out of host memory");
    d->device = device;
    d->S = n_scores;
    d->ND = ND;
    d->no_scale = no_scale;
    d->n_desc = n_desc;
    HIP_TRY(d->d_F.alloc(NPS_MULTI_MAX_SCORES));
    HIP_TRY(hipMemcpy(d->d_F.get(), F, sizeof(int) * n_scores, hipMemcpyHostToDevice));
    if (n_desc) HIP_TRY(upload_desc(d->d_desc, rows, n_desc * n_scores));
    *out = owner.release();
    return NPS_OK;
}

extern "C" int nps_multidef_create(nps_multidef **out, int device, const nps_row_desc *rows, int n_scores,
                                   uint64_t n_desc) {
    return nps_multidef_create_bits(out, device, rows, n_scores, n_desc, 0);
}

extern "C" void nps_multidef_destroy(nps_multidef *d) { delete d; }

struct nps_multi {
    Stream stream;  // (first: destroyed last)
    int device = 0, S = 0, cus = 0;
    uint64_t n = 0;
    nps_params params{};
    DevBuf<unsigned char> d_state;  // MultiState[S]
    DevBuf<double> d_part;          // [S][n] float64 running sums
    bool have_sums = false;
    DevBuf<unsigned char> d_table;  // the weight table and its flags (bytes), grown on demand
    DevBuf<int32_t> d_partial;      // grown on demand
    DevBuf<double> d_offsets, d_scores;
    Event ev[4];
    double ms[3] = {0.0, 0.0, 0.0};  // params, product, fold of all calls since the last reset
    bool timed = false;
    int coarse_missing = 0;          // nps_multi_set_missing_weight_bits: leading base-256 digits kept (4 = 32 bits, 5 = 40; 0 = all)
    bool broken = false;             // a HIP call failed between the first and the last launch of a pass
    // dosage cohorts (nps_multi_ds.hip), grown on demand: the row tallies and the (row, score) records of the last such
    // pass, the partial planes of its row chunks
    DevBuf<MultiDsTally> d_ds_tally;
    DevBuf<DsRowP> d_ds_rowp;
    DevBuf<double> d_ds_planes;
    uint64_t ds_rows = 0;            // rows of the most recent call if it was on a dosage cohort (nps_multi_row_tallies)
    bool ds_last = false;

    ~nps_multi() {  // queued work may still use what the members release
        (void)hipSetDevice(device);
        if (stream.get()) (void)hipStreamSynchronize(stream.get());
    }
};

// add the device time of the last call (if its events have not been read yet) to the running totals
static void multi_drain_timing(nps_multi *m) {
    if (!m->timed) return;
    float a = 0.f, b = 0.f, c = 0.f;
    if (hipEventSynchronize(m->ev[3].get()) == hipSuccess) {
        (void)hipEventElapsedTime(&a, m->ev[0].get(), m->ev[1].get());
        (void)hipEventElapsedTime(&b, m->ev[1].get(), m->ev[2].get());
        (void)hipEventElapsedTime(&c, m->ev[2].get(), m->ev[3].get());
        m->ms[0] += a;
        m->ms[1] += b;
        m->ms[2] += c;
    }
    m->timed = false;
}

extern "C" int nps_multi_create(nps_multi **out, int device, uint64_t n_samples, const nps_params *params,
                                int n_scores) {
    if (!out) return fail(NPS_E_INVAL, "out is NULL");
    *out = nullptr;
    int rc = check_params(params);
    if (rc) return rc;
    if (n_scores < 1 || n_scores > NPS_MULTI_MAX_SCORES)
        return fail(NPS_E_INVAL, "n_scores %d outside 1..%d", n_scores, NPS_MULTI_MAX_SCORES);
    if (n_samples > 0x7fffffffull) return fail(NPS_E_UNSUPPORTED, "n_samples too large");
    rc = select_device(device);
    if (rc) return rc;
    std::unique_ptr<nps_multi> owner(new (std::nothrow) nps_multi);
    nps_multi *m = owner.get();
    if (!m) return fail(NPS_E_NOMEM, "out of host memory");
    m->device = device;
    m->S = n_scores;
    m->n = n_samples;
    m->params = *params;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    m->cus = prop.multiProcessorCount;
    const size_t sb = multi_state_bytes() * NPS_MULTI_MAX_SCORES;
    HIP_TRY(m->stream.create());
    HIP_TRY(m->d_state.alloc(sb));
    HIP_TRY(hipMemset(m->d_state.get(), 0, sb));
    HIP_TRY(m->d_part.alloc(std::max<uint64_t>(n_samples, 1) * n_scores));
    HIP_TRY(m->d_scores.alloc(std::max<uint64_t>(n_samples, 1) * n_scores));
    HIP_TRY(m->d_offsets.alloc(NPS_MULTI_MAX_SCORES));
    for (int k = 0; k < 4; ++k) HIP_TRY(m->ev[k].create(hipEventDefault));
    *out = owner.release();
    return NPS_OK;
}

extern "C" void nps_multi_destroy(nps_multi *m) { delete m; }

extern "C" int nps_multi_set_missing_weight_bits(nps_multi *m, int bits) {
    if (!m) return fail(NPS_E_INVAL, "ctx is NULL");
    if (bits != 0 && bits != 32 && bits != 40 && bits != 56)
        return fail(NPS_E_INVAL, "bits must be 32, 40 or 56 (0 = default 56), not %d", bits);
    m->coarse_missing = bits == 32 ? 4 : bits == 40 ? 5 : 0;
    return NPS_OK;
}

extern "C" int nps_multi_reset(nps_multi *m, const nps_params *params) {
    if (!m) return fail(NPS_E_INVAL, "ctx is NULL");
    if (params) {
        int rc = check_params(params);
        if (rc) return rc;
        m->params = *params;
    }
    HIP_TRY(hipSetDevice(m->device));
    multi_drain_timing(m);
    HIP_TRY(hipMemsetAsync(m->d_state.get(), 0, multi_state_bytes() * NPS_MULTI_MAX_SCORES, m->stream.get()));
    m->broken = false;
    m->have_sums = false;
    m->ds_last = false;
    m->ds_rows = 0;
    m->ms[0] = m->ms[1] = m->ms[2] = 0.0;
    return NPS_OK;
}

// A dosage cohort (nps_multi_ds.hip): one tally read of the rows, one accumulation read for all S scores.  The caller has
// checked the arguments and made the device current.  nps_multi_set_missing_weight_bits has no meaning here: float64.
static int multi_score_ds(nps_multi *m, const nps_cohort *co, uint64_t cohort_row0, const nps_multidef *def) {
    const uint64_t rows = def->n_desc;
    const int elem = co->format == NPS_FMT_DS16 ? 2 : 4;
    const uint64_t stride_e = co->stride_bytes / elem;
    const void *ds = (const char *)co->d_data.get() + cohort_row0 * co->stride_bytes;
    const MultiDsPlan pl = multi_ds_plan(m->n, rows, m->cus);
    if (rows > 0x7fffffffull) return fail(NPS_E_UNSUPPORTED, "too many rows for one call");
    HIP_TRY(m->d_ds_tally.ensure(rows, m->stream.get()));
    HIP_TRY(m->d_ds_rowp.ensure(rows * m->S, m->stream.get()));
    HIP_TRY(m->d_ds_planes.ensure(pl.plane_elems(m->S), m->stream.get()));
    if (m->timed && hipEventQuery(m->ev[3].get()) == hipSuccess) multi_drain_timing(m);
    m->timed = false;
    // Everything that can be refused has been checked and allocated (see nps_score_cohort_multi).
    auto run = [&]() -> hipError_t {
        hipError_t e = hipEventRecord(m->ev[0].get(), m->stream.get());
        if (e != hipSuccess) return e;
        e = launch_multi_ds_tally(m->stream.get(), ds, elem, stride_e, m->n, rows, m->d_ds_tally.get());
        if (e != hipSuccess) return e;
        e = launch_multi_ds_params(m->stream.get(), m->d_ds_tally.get(), def->d_desc.get(), rows, m->S, m->n, dev_params(m->params),
                                   m->d_ds_rowp.get(), m->d_state.get());
        if (e != hipSuccess) return e;
        e = hipEventRecord(m->ev[1].get(), m->stream.get());
        if (e != hipSuccess) return e;
        e = launch_multi_ds_accumulate(m->stream.get(), pl, ds, elem, stride_e, m->n, m->d_ds_rowp.get(), rows, m->S,
                                       m->d_ds_planes.get());
        if (e != hipSuccess) return e;
        e = hipEventRecord(m->ev[2].get(), m->stream.get());
        if (e != hipSuccess) return e;
        e = launch_multi_ds_fold(m->stream.get(), pl, m->d_ds_planes.get(), m->n, m->S, m->d_part.get(), m->have_sums ? 0 : 1);
        if (e != hipSuccess) return e;
        return hipEventRecord(m->ev[3].get(), m->stream.get());
    };
    const hipError_t e = run();
    if (e != hipSuccess) {
        m->broken = true;
        return fail(NPS_E_HIP, "nps_score_cohort_multi: %s (context needs nps_multi_reset)", hipGetErrorString(e));
    }
    m->have_sums = true;
    m->timed = true;
    m->ds_last = true;
    m->ds_rows = rows;
    return NPS_OK;
}

extern "C" int nps_score_cohort_multi(nps_multi *m, const nps_cohort *co, uint64_t cohort_row0,
                                      const nps_multidef *def) {
    if (!m || !co || !def) return fail(NPS_E_INVAL, "ctx, cohort or definitions is NULL");
    if (m->broken) return fail(NPS_E_STATE, "an earlier pass failed on the device: nps_multi_reset first");
    const bool is_ds = co->format == NPS_FMT_DS32 || co->format == NPS_FMT_DS16;
    if (co->format != NPS_FMT_GT2M && !is_ds)
        return fail(NPS_E_INVAL, "nps_score_cohort_multi needs a NPS_FMT_GT2M, NPS_FMT_DS32 or NPS_FMT_DS16 cohort");
    if (co->device != m->device || def->device != m->device)
        return fail(NPS_E_INVAL, "cohort / definitions / context on different devices");
    if (co->n_samples != m->n)
        return fail(NPS_E_INVAL, "cohort has %llu samples, context %llu", (unsigned long long)co->n_samples,
                    (unsigned long long)m->n);
    if (def->S != m->S) return fail(NPS_E_INVAL, "definitions hold %d scores, context %d", def->S, m->S);
    if (cohort_row0 & 127) return fail(NPS_E_INVAL, "cohort_row0 must be a multiple of 128");
    int rc = check_range(co, cohort_row0, def->n_desc);
    if (rc) return rc;
    if (def->n_desc == 0) return NPS_OK;
    if (!is_ds && def->no_scale >= 0)
        return fail(NPS_E_UNSUPPORTED, "score %d: the weight bound max|beta| (3 + max(2, 2 max|eaf|)) is not finite, beyond "
                    "the fixed-point weights of a NPS_FMT_GT2M pass; score this definition on a dosage cohort or with the "
                    "single-score path (nps_scoredef_create / nps_score_cohort_def)", def->no_scale);
    HIP_TRY(hipSetDevice(m->device));
    if (is_ds) {
        rc = cohort_quiesce(co);  // rows pushed into the cohort (nps_cohort_push_pl) are complete
        if (rc) return rc;
        return multi_score_ds(m, co, cohort_row0, def);
    }
    const MultiPlan pl = multi_plan(m->n, def->n_desc, m->S, def->ND, m->coarse_missing, m->cus);
    HIP_TRY(m->d_table.ensure(pl.table_bytes() + pl.flag_bytes(), m->stream.get()));
    HIP_TRY(m->d_partial.ensure(pl.partial_elems(), m->stream.get()));
    // (the timing events are about to be re-recorded: read the previous pass's times only if it has completed already --
    //  a caller that queues pass after pass is never blocked here; its per-pass times are then not accumulated)
    if (m->timed && hipEventQuery(m->ev[3].get()) == hipSuccess) multi_drain_timing(m);
    m->timed = false;
    // Everything that can be refused has been checked and allocated.  From here a HIP failure leaves the running
    // sums and counts of the context undefined: it is marked broken (NPS_E_STATE until nps_multi_reset).
    // (multi_params_kernel writes every fragment of the table, zeros for unused columns and padding rows)
    auto run = [&]() -> hipError_t {
        hipError_t e = hipEventRecord(m->ev[0].get(), m->stream.get());
        if (e != hipSuccess) return e;
        e = launch_multi_params(m->stream.get(), co->d_row_tally.get() + cohort_row0, def->d_desc.get(), def->n_desc, m->S, pl, m->n,
                                dev_params(m->params), def->d_F.get(), m->d_table.get(), m->d_state.get(), m->coarse_missing);
        if (e != hipSuccess) return e;
        e = hipEventRecord(m->ev[1].get(), m->stream.get());
        if (e != hipSuccess) return e;
        if (m->n) {
            e = launch_multi_mfma(m->stream.get(), pl, co->d_data.get(), cohort_row0 / 128, m->d_table.get(), m->d_partial.get(), m->d_state.get(),
                                  co->d_row_tally.get() + cohort_row0, def->n_desc,
                                  reinterpret_cast<uint32_t *>(m->d_table.get() + pl.table_bytes()));
            if (e != hipSuccess) return e;
        }
        e = hipEventRecord(m->ev[2].get(), m->stream.get());
        if (e != hipSuccess) return e;
        e = launch_multi_fold(m->stream.get(), pl, m->d_partial.get(), m->n, m->S, def->d_F.get(), m->d_part.get(), m->have_sums ? 0 : 1,
                              m->d_state.get());
        if (e != hipSuccess) return e;
        return hipEventRecord(m->ev[3].get(), m->stream.get());
    };
    const hipError_t e = run();
    if (e != hipSuccess) {
        m->broken = true;
        return fail(NPS_E_HIP, "nps_score_cohort_multi: %s (context needs nps_multi_reset)", hipGetErrorString(e));
    }
    m->have_sums = true;
    m->timed = true;
    m->ds_last = false;
    return NPS_OK;
}

extern "C" int nps_multi_row_tallies(nps_multi *m, uint64_t first, uint64_t n, uint64_t *nmissing_out, double *sum_out,
                                     double *sum_flipped_out) {
    if (!m) return fail(NPS_E_INVAL, "ctx is NULL");
    if (m->broken) return fail(NPS_E_STATE, "an earlier pass failed on the device: nps_multi_reset first");
    if (!m->ds_last)
        return fail(NPS_E_STATE, "nps_multi_row_tallies: the most recent nps_score_cohort_multi call of this context was not "
                                 "on a NPS_FMT_DS32 / NPS_FMT_DS16 cohort (or the context was reset since)");
    if (first > m->ds_rows || n > m->ds_rows - first)
        return fail(NPS_E_INVAL, "rows %llu + %llu outside the %llu rows of the last pass", (unsigned long long)first,
                    (unsigned long long)n, (unsigned long long)m->ds_rows);
    if (n == 0) return NPS_OK;
    HIP_TRY(hipSetDevice(m->device));
    std::vector<MultiDsTally> t(n);
    HIP_TRY(hipMemcpyAsync(t.data(), m->d_ds_tally.get() + first, sizeof(MultiDsTally) * n, hipMemcpyDeviceToHost, m->stream.get()));
    HIP_TRY(hipStreamSynchronize(m->stream.get()));
    for (uint64_t j = 0; j < n; ++j) {
        if (nmissing_out) nmissing_out[j] = t[j].nmiss;
        if (sum_out) sum_out[j] = t[j].sum;
        if (sum_flipped_out) sum_flipped_out[j] = t[j].sum_flipped;
    }
    return NPS_OK;
}

extern "C" int nps_multi_geometry(const nps_multi *m, int format, uint64_t n_rows, uint32_t *row_chunks, uint32_t *rows_per_chunk) {
    if (!m) return fail(NPS_E_INVAL, "ctx is NULL");
    if (format == NPS_FMT_GT2M) return fail(NPS_E_UNSUPPORTED, "nps_multi_geometry reports the plan of dosage cohorts");
    if (format != NPS_FMT_DS32 && format != NPS_FMT_DS16) return fail(NPS_E_INVAL, "format %d is not a dosage format", format);
    const MultiDsPlan pl = multi_ds_plan(m->n, n_rows, m->cus);  // (one plan for both element types)
    if (row_chunks) *row_chunks = pl.n_chunks;
    if (rows_per_chunk) *rows_per_chunk = (uint32_t)std::min<uint64_t>(pl.rows_per_chunk, 0xffffffffull);
    return NPS_OK;
}

static int multi_finish_common(nps_multi *m, const double *offsets, double *d_dst, double *h_scores_out,
                               uint64_t *nloci_out, int normalise = 1) {
    if (!offsets && normalise) return fail(NPS_E_INVAL, "offsets is NULL");
    if (m->broken) return fail(NPS_E_STATE, "an earlier pass failed on the device: nps_multi_reset first");
    HIP_TRY(hipSetDevice(m->device));
    if (normalise)
        HIP_TRY(hipMemcpyAsync(m->d_offsets.get(), offsets, sizeof(double) * m->S, hipMemcpyHostToDevice, m->stream.get()));
    HIP_TRY(launch_multi_finish(m->stream.get(), m->d_part.get(), m->n, m->S, m->d_state.get(), m->d_offsets.get(), m->have_sums ? 1 : 0,
                                d_dst, normalise));
    std::vector<char> st(multi_state_bytes() * m->S);
    HIP_TRY(hipMemcpyAsync(st.data(), m->d_state.get(), st.size(), hipMemcpyDeviceToHost, m->stream.get()));
    if (h_scores_out && m->n)
        HIP_TRY(hipMemcpyAsync(h_scores_out, d_dst, sizeof(double) * m->n * m->S, hipMemcpyDeviceToHost, m->stream.get()));
    HIP_TRY(hipStreamSynchronize(m->stream.get()));
    if (nloci_out)
        for (int s = 0; s < m->S; ++s)
            memcpy(&nloci_out[s], st.data() + multi_state_bytes() * s, sizeof(uint64_t));  // first field
    return NPS_OK;
}

extern "C" int nps_multi_finish(nps_multi *m, const double *offsets, double *scores_out, uint64_t *nloci_out) {
    if (!m) return fail(NPS_E_INVAL, "ctx is NULL");
    if (m->n && !scores_out) return fail(NPS_E_INVAL, "scores_out is NULL");
    return multi_finish_common(m, offsets, m->d_scores.get(), scores_out, nloci_out);
}

extern "C" int nps_multi_finish_device(nps_multi *m, const double *offsets, double *d_scores_out,
                                       uint64_t *nloci_out) {
    if (!m) return fail(NPS_E_INVAL, "ctx is NULL");
    if (m->n && !d_scores_out) return fail(NPS_E_INVAL, "d_scores_out is NULL");
    return multi_finish_common(m, offsets, d_scores_out, nullptr, nloci_out);
}

extern "C" int nps_multi_n_scores(const nps_multi *m) { return m ? m->S : 0; }
extern "C" uint64_t nps_multi_n_samples(const nps_multi *m) { return m ? m->n : 0; }
extern "C" int nps_multi_device(const nps_multi *m) { return m ? m->device : -1; }

extern "C" int nps_multi_partial_device(nps_multi *m, double *d_sums_out, uint64_t *nloci_out) {
    if (!m) return fail(NPS_E_INVAL, "ctx is NULL");
    if (m->n && !d_sums_out) return fail(NPS_E_INVAL, "d_sums_out is NULL");
    return multi_finish_common(m, nullptr, d_sums_out, nullptr, nloci_out, 0);
}

extern "C" int nps_multi_partial(nps_multi *m, double *sums_out, uint64_t *nloci_out) {
    if (!m) return fail(NPS_E_INVAL, "ctx is NULL");
    if (m->n && !sums_out) return fail(NPS_E_INVAL, "sums_out is NULL");
    return multi_finish_common(m, nullptr, m->d_scores.get(), sums_out, nloci_out, 0);
}

extern "C" int nps_multi_timing(nps_multi *m, double *ms_params, double *ms_product, double *ms_fold) {
    if (!m) return fail(NPS_E_INVAL, "ctx is NULL");
    HIP_TRY(hipSetDevice(m->device));
    multi_drain_timing(m);
    if (ms_params) *ms_params = m->ms[0];
    if (ms_product) *ms_product = m->ms[1];
    if (ms_fold) *ms_fold = m->ms[2];
    return NPS_OK;
}

// ------------------------------------------------------------------------------------------
extern "C" int nps_profile_enable(nps_ctx *c, int on) {
    if (!c) return fail(NPS_E_INVAL, "ctx is NULL");
    c->profiling = on != 0;
    return NPS_OK;
}

extern "C" int nps_profile_get(nps_ctx *c, nps_profile *out, int reset) {
    if (!c || !out) return fail(NPS_E_INVAL, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream.get()));
    resolve_spans(c);
    *out = c->prof;
    if (reset) c->prof = nps_profile{};
    return NPS_OK;
}

extern "C" void *nps_stream(nps_ctx *c) { return c ? (void *)c->stream.get() : nullptr; }

extern "C" int nps_fused_geometry(nps_ctx *c, int format, uint64_t n_rows, uint32_t *slices,
                                  uint32_t *teams, uint32_t *samples_per_slice) {
    if (!c) return fail(NPS_E_INVAL, "ctx is NULL");
    const int ds_elem = format == NPS_FMT_DS16 ? 2 : 4;
    if (format == NPS_FMT_DS16) format = NPS_FMT_DS32;  // (the same kernel and slices; four rows per batch)
    if (format != NPS_FMT_GT2 && format != NPS_FMT_DS32 && format != NPS_FMT_GT2X)
        return fail(NPS_E_INVAL, "unknown format %d", format);
    HIP_TRY(hipSetDevice(c->device));
    if (format == NPS_FMT_GT2X) {
        MxPlan mp;
        HIP_TRY(mx_plan(c->device, c->n, n_rows, false, &mp));
        // (more strips than compute units: the grid of the accumulation with given tallies -- kept with the cohort, or from
        //  the tally pass; its slices are still the 2048-sample strips)
        if (mp.ok && mp.given) HIP_TRY(mx_plan(c->device, c->n, n_rows, true, &mp));
        // (the single-read kernel may cut its own strips of 62 units = 1 984 samples from the unit sequence: what the grid IS)
        if (slices) *slices = mp.ok ? mp.grid_P : 0;
        if (teams) *teams = mp.ok ? mp.Q : 0;
        if (samples_per_slice) *samples_per_slice = mp.ok ? 32 * mp.grid_U : 0;
        return NPS_OK;
    }
    FusedPlan plan;
    if (format == NPS_FMT_DS32)
        HIP_TRY(ds_fused_plan(c->device, c->n, n_rows, 0, 0, &plan, ds_elem));
    else
        HIP_TRY(fused_plan(c->device, c->n, n_rows, 0, 0, &plan));
    if (slices) *slices = plan.ok ? plan.P : 0;
    if (teams) *teams = plan.ok ? plan.Q : 0;
    if (samples_per_slice)
        *samples_per_slice = !plan.ok ? 0 : (format == NPS_FMT_DS32 ? (plan.threads - 64) * 8 : (plan.threads - 64) * 16);
    return NPS_OK;
}
