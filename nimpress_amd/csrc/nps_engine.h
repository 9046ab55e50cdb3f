// nps_engine.h -- what the units that implement the C-ABI of include/nps.h share (internal: no kernel source sees it).
//
// One unit per object: nps_engine.hip (errors, device selection, nps_ctx and everything streamed through it),
// nps_cohort.hip (nps_cohort), nps_resident.hip (nps_scoredef, nps_sampleset, nps_samplegroups, scoring a resident cohort) and
// nps_multiscore.hip (nps_multidef, nps_multi).  Here: the objects' structs, HIP_TRY, the one row path through a staging
// ring with the checks of a pushed row (inline: a per-row push makes no call into another unit), and the declarations of
// the helpers one unit has for the others -- hidden, so that the library exports what it did as one unit.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "nps_kernels.h"
#include "nps_own.h"

using namespace nps;

#pragma GCC visibility push(hidden)
// ---- nps_engine.hip
int fail(int code, const char *fmt, ...);  // the text of nps_last_error() on this thread; returns code
int select_device(int device);
int check_params(const nps_params *p);
DevParams dev_params(const nps_params &p);
int check_usable(nps_ctx *c);
int check_sampleset(const nps_ctx *c, const nps_sampleset *s);
int check_ungrouped(const nps_ctx *c, const char *what);
int ensure_all_chunks(nps_ctx *c);
int run_batch(nps_ctx *c);
int materialize_resident_stats(nps_ctx *c);
void host_locus_row(nps_ctx *c, int kind, int rie, double beta, double eaf, nps_locus_stat *st);
// ---- nps_cohort.hip
int check_range(const nps_cohort *c, uint64_t row0, uint64_t nrows);
int cohort_quiesce(const nps_cohort *c);
bool mx_tallies_valid(const nps_cohort *c, uint64_t sb0, uint64_t n_sb);
void mx_tallies_mark(nps_cohort *c, uint64_t sb0, uint64_t n_sb, bool valid);
hipError_t mx_tallies_alloc(nps_cohort *c);
int mx_keep_tallies_locked(nps_cohort *c);
// ---- nps_resident.hip
hipError_t upload_desc(DevBuf<nps_row_desc> &d, const nps_row_desc *rows, uint64_t n);
#pragma GCC visibility pop

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return fail(_e == hipErrorOutOfMemory ? NPS_E_NOMEM : NPS_E_HIP, "%s failed: %s",  \
                        #expr, hipGetErrorString(_e));                                         \
    } while (0)

// nps_ctx::d_nloci, the device's result block as nps_reset zeroes it and a grouped finish fetches it: [0] used rows, [1] status
// bits, [kGroupNloci .. + 8) the rows used per group of a grouped context
constexpr size_t kResultWords = 16, kGroupNloci = 8;

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

// A partition of a cohort's samples into groups (nps_score_cohort_def_groups): the labels of nps_group_labels.h on the
// device, immutable after creation -- contexts on several threads may share one.
struct nps_samplegroups {
    int device = 0;
    int n_groups = 0;
    uint64_t n_samples = 0;
    uint64_t size[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    DevBuf<unsigned char> d_label;        // one byte per sample, padded with 255 to a multiple of 64 (tally, accumulation, finish)
    DevBuf<unsigned char> d_present;      // one byte per 256 samples: the groups that occur there (the tally)
    DevBuf<unsigned long long> d_size;    // [n_groups] (the rows' decisions)

    ~nps_samplegroups() {  // queued work may still read the labels
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
    // grouped runs (nps_score_cohort_def_groups): the context is "grouped" from its first such call until nps_reset, with
    // ONE groups object; plain_rows: it has taken ungrouped rows since its last reset (the two do not mix)
    const nps_samplegroups *groups = nullptr;
    bool plain_rows = false;
    DevBuf<DsTally> d_grp_tally;          // [rows][n_groups]
    DevBuf<GroupRowP> d_grp_rowp;         // [rows]
    DevBuf<double> d_grp_imp;             // [rows][8]
    DevBuf<nps_locus_stat> d_grp_stats;   // [rows][n_groups]; entries of a run wait here like d_rstats' (res_pending)

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
    DevBuf<unsigned long long> d_nloci;      // [0] used rows counted on the device, [1] sticky status bits, [8 .. 15] per group
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
static inline void stage_bed_row(void *slot, const uint8_t *bed_row, uint64_t n) {
    const size_t bytes = (size_t)((n + 3) / 4), padded = sizeof(uint32_t) * words_for(n);
    memcpy(slot, bed_row, bytes);
    memset((char *)slot + bytes, 0, padded - bytes);
}

// the typed GT vector of a record; max_ploidy: what the destination holds
static inline int check_raw_gt(int elem_bytes, int ploidy, int eaidx, int max_ploidy) {
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4)
        return fail(NPS_E_INVAL, "elem_bytes %d (1, 2 or 4)", elem_bytes);
    if (ploidy < 1) return fail(NPS_E_INVAL, "ploidy %d < 1", ploidy);
    if (ploidy > max_ploidy)
        return max_ploidy == 2 ? fail(NPS_E_UNSUPPORTED, "ploidy %d > 2 does not fit the 2-bit cohort", ploidy)
                               : fail(NPS_E_UNSUPPORTED, "ploidy %d > 8", ploidy);
    if (eaidx < 0) return fail(NPS_E_INVAL, "eaidx %d < 0 (nimpress.nim:380 doAssert)", eaidx);
    return NPS_OK;
}

// the typed FORMAT/PL vector of a diploid record with n_alleles alleles (REF + ALTs)
static inline int check_raw_pl(int elem_bytes, int n_alleles, int eaidx) {
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4)
        return fail(NPS_E_INVAL, "elem_bytes %d (1, 2 or 4)", elem_bytes);
    if (n_alleles < 2 || n_alleles > 8) return fail(NPS_E_UNSUPPORTED, "FORMAT/PL of %d alleles (2 .. 8)", n_alleles);
    if (eaidx < 0 || eaidx >= n_alleles) return fail(NPS_E_INVAL, "eaidx %d outside the %d alleles", eaidx, n_alleles);
    return NPS_OK;
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

#ifdef NPS_DIAGNOSTICS
// run-time switches exist in diagnostics builds only (tools/mkexp.sh -DNPS_DIAGNOSTICS): the release
// library reads no environment variable on its launch path
static inline uint64_t env_u64(const char *name, uint64_t dflt) {
    const char *s = getenv(name);
    if (!s || !*s) return dflt;
    char *end = nullptr;
    unsigned long long v = strtoull(s, &end, 10);
    return end && *end == 0 ? (uint64_t)v : dflt;
}
#else
static inline uint64_t env_u64(const char *, uint64_t dflt) { return dflt; }
#endif

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
