// nps_engine.hip -- the C-ABI of include/nps.h, first of four units (nps_engine.h): errors, device selection, and the
// streaming context nps_ctx: create / reset / destroy, every row push, flush, finish, partial sums, profile, geometry.
// The other objects live in nps_cohort.hip, nps_resident.hip and nps_multiscore.hip.
//
// Host-side orchestration only: staging, batching, launches, bookkeeping of per-row stats.  All
// per-sample arithmetic happens in nps_kernels.hip (and nps_fused.hip).  There is no CPU compute
// path here: if HIP is unusable every entry point that would compute returns NPS_E_NODEVICE.
#include <cstdarg>
#include <cstdio>
#include <new>
#include <string>

#include "nps_engine.h"

extern "C" int64_t nps_live_resources(void) { return live_resources.load(); }

// ------------------------------------------------------------------------------------------
// errors (the one definition: every unit reports through fail)
static thread_local std::string g_last_error;

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

DevParams dev_params(const nps_params &p) {
    DevParams d;
    d.imp_locus = p.imp_locus;
    d.imp_missing = p.imp_missing;
    d.imp_sample = p.imp_sample;
    d.max_missing_rate = p.max_missing_rate;
    d.min_cs = (double)p.min_cs;
    return d;
}

int check_params(const nps_params *p) {
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

__global__ void warmup_kernel(unsigned int *p) {  // (the only kernel of the four units)
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

int select_device(int device) {
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
    HIP_TRY(hipMemsetAsync(c->d_nloci.get(), 0, kResultWords * sizeof(unsigned long long), c->stream.get()));
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
    c->groups = nullptr;
    c->plain_rows = false;
    return NPS_OK;
}

// the two-pass kernels add into every chunk of d_part: zero the chunks nothing has written yet
int ensure_all_chunks(nps_ctx *c) {
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
void host_locus_row(nps_ctx *c, int kind, int rie, double beta, double eaf,
                           nps_locus_stat *st) {
    const RowDecision d = no_data_row(dev_params(c->params), kind, eaf, rie != 0);
    *st = row_stat(d, 0, 0, 0.0);
    if (d.used) {
        volatile double term = d.imp * beta;  // same product as nimpress.nim:640, not contracted
        c->const_sum += term;
        c->host_nloci += 1;
    }
}

int check_usable(nps_ctx *c) {
    if (!c) return fail(NPS_E_INVAL, "ctx is NULL");
    if (c->broken)
        return fail(NPS_E_STATE, "a previous call on this context failed half-way through its launches; "
                                 "call nps_reset before using it again");
    return NPS_OK;
}

// A grouped context (nps_score_cohort_def_groups) takes grouped calls only until nps_reset
int check_ungrouped(const nps_ctx *c, const char *what) {
    if (c->groups)
        return fail(NPS_E_STATE, "%s on a context that scores sample groups (nps_score_cohort_def_groups); nps_reset first", what);
    return NPS_OK;
}

// run the open batch: params -> accumulate; then collect its stats
int run_batch(nps_ctx *c) {
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
    c->plain_rows = true;
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
    if (int grc = check_ungrouped(c, "nps_push_pl")) return grc;
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
    if (int grc = check_ungrouped(c, "nps_push_gt")) return grc;
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
    if (int grc = check_ungrouped(c, "nps_push_packed")) return grc;
    if (c->n && !row) return fail(NPS_E_INVAL, "row is NULL");
    return push_2bit(c, row, -1, ref_is_effect, beta, eaf);
}

extern "C" int nps_push_bed(nps_ctx *c, const uint8_t *bed_row, int effect_is_a1, int ref_is_effect,
                            double beta, double eaf) {
    if (int urc = check_usable(c)) return urc;
    if (int grc = check_ungrouped(c, "nps_push_bed")) return grc;
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
    if (int grc = check_ungrouped(c, "nps_push_ds")) return grc;
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
    if (int grc = check_ungrouped(c, "nps_push_locus")) return grc;
    if (kind != NPS_ROW_UNCOVERED && kind != NPS_ROW_ABSENT && kind != NPS_ROW_FILTERED)
        return fail(NPS_E_INVAL, "kind %d is not a no-data row kind", kind);
    PendingRow p;
    p.batch_idx = -1;
    p.is_ds = 0;
    host_locus_row(c, kind, ref_is_effect, beta, eaf, &p.host);
    c->pending.push_back(p);
    c->plain_rows = true;
    return NPS_OK;
}

// the device's result block (used rows, status bits) -> pinned host copy; the caller synchronises
// (words: 3, or kResultWords with the groups' counts)
static int fetch_result(nps_ctx *c, size_t words = 3) {
    HIP_TRY(hipMemcpyAsync(c->h_result, c->d_nloci.get(), words * sizeof(unsigned long long), hipMemcpyDeviceToHost,
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

// nps_flush and nps_flush_groups: the rows -- of a grouped context the (row, group) entries -- completed and copied out
static int flush_common(nps_ctx *c, nps_locus_stat *stats_out, size_t cap, size_t *n_out) {
    int rc = NPS_OK;
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

extern "C" int nps_flush(nps_ctx *c, nps_locus_stat *stats_out, size_t cap, size_t *n_out) {
    int rc = check_usable(c);
    if (rc) return rc;
    if (stats_out && (rc = check_ungrouped(c, "nps_flush with stats_out"))) return rc;
    return flush_common(c, stats_out, cap, n_out);
}

extern "C" int nps_flush_groups(nps_ctx *c, nps_locus_stat *stats_out, size_t cap, size_t *n_out) {
    int rc = check_usable(c);
    if (rc) return rc;
    if (!c->groups) return fail(NPS_E_STATE, "nps_flush_groups on a context that has taken no grouped call since its last reset");
    return flush_common(c, stats_out, cap, n_out);
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
    if ((rc = check_ungrouped(c, "nps_finish"))) return rc;
    if (c->n && !scores_out) return fail(NPS_E_INVAL, "scores_out is NULL");
    HIP_TRY(hipSetDevice(c->device));
    return finish_common(c, offset, c->d_scores.get(), scores_out, nloci_out);
}

extern "C" int nps_finish_device(nps_ctx *c, double offset, double *d_scores_out,
                                 uint64_t *nloci_out) {
    int rc = check_usable(c);
    if (rc) return rc;
    if ((rc = check_ungrouped(c, "nps_finish_device"))) return rc;
    if (c->n && !d_scores_out) return fail(NPS_E_INVAL, "d_scores_out is NULL");
    HIP_TRY(hipSetDevice(c->device));
    return finish_common(c, offset, d_scores_out, nullptr, nloci_out);
}

// nps_finish for the kept samples of a set: finish_kernel makes every sample's score as nps_finish does (the same
// arithmetic, so a set that keeps everybody returns nps_finish's bits), the gather takes the kept ones, in cohort
// order, into d_dst[n_kept]
int check_sampleset(const nps_ctx *c, const nps_sampleset *s) {
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
    if ((rc = check_ungrouped(c, "nps_finish_subset"))) return rc;
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
    if ((rc = check_ungrouped(c, "nps_finish_subset"))) return rc;
    rc = check_sampleset(c, s);
    if (rc) return rc;
    if (!d_scores_out) return fail(NPS_E_INVAL, "d_scores_out is NULL");
    HIP_TRY(hipSetDevice(c->device));
    return finish_subset_common(c, s, offset, d_scores_out, nullptr, nloci_out);
}

extern "C" int nps_partial_device(nps_ctx *c, double *d_sums_out, uint64_t *nloci_out) {
    int rc = check_usable(c);
    if (rc) return rc;
    if ((rc = check_ungrouped(c, "nps_partial_device"))) return rc;
    if (c->n && !d_sums_out) return fail(NPS_E_INVAL, "d_sums_out is NULL");
    HIP_TRY(hipSetDevice(c->device));
    return finish_common(c, 0.0, d_sums_out, nullptr, nloci_out, false);
}

// nps_finish for every group of a grouped context: one enqueue and one synchronisation like finish_common, the groups' counts
// of used rows in the same copy as the status block
static int finish_groups_common(nps_ctx *c, const nps_samplegroups *g, double offset, double *d_dst, double *h_scores_out,
                                uint64_t *nloci_out) {
    {
        ProfScope ps(c, P_REDUCE);
        HIP_TRY(launch_groups_finish(c->stream.get(), c->d_part.get(), c->chunks_used, c->geom.part_chunk_stride, c->n, c->const_sum,
                                     g->d_label.get(), c->d_nloci.get() + kGroupNloci, c->host_nloci, offset, d_dst));
    }
    int rc = fetch_result(c, kResultWords);
    if (rc) return rc;
    if (h_scores_out)
        HIP_TRY(hipMemcpyAsync(h_scores_out, d_dst, sizeof(double) * c->n, hipMemcpyDeviceToHost, c->stream.get()));
    HIP_TRY(hipStreamSynchronize(c->stream.get()));
    rc = check_status(c);
    if (rc) return rc;
    if (nloci_out)
        for (int k = 0; k < g->n_groups; ++k) nloci_out[k] = c->host_nloci + c->h_result[kGroupNloci + k];
    return NPS_OK;
}

// the groups object of a grouped context's calls: the one its first grouped call named
static int check_groups_of(const nps_ctx *c, const nps_samplegroups *g, const char *what) {
    if (!g) return fail(NPS_E_INVAL, "groups is NULL");
    if (!c->groups) return fail(NPS_E_STATE, "%s on a context that has taken no grouped call since its last reset", what);
    if (g != c->groups) return fail(NPS_E_INVAL, "%s: not the groups object this context scores (one per context until nps_reset)", what);
    return NPS_OK;
}

extern "C" int nps_finish_groups(nps_ctx *c, const nps_samplegroups *g, double offset, double *scores_out, uint64_t *nloci_out) {
    int rc = check_usable(c);
    if (rc) return rc;
    rc = check_groups_of(c, g, "nps_finish_groups");
    if (rc) return rc;
    if (!scores_out) return fail(NPS_E_INVAL, "scores_out is NULL");
    HIP_TRY(hipSetDevice(c->device));
    return finish_groups_common(c, g, offset, c->d_scores.get(), scores_out, nloci_out);
}

extern "C" int nps_finish_groups_device(nps_ctx *c, const nps_samplegroups *g, double offset, double *d_scores_out,
                                        uint64_t *nloci_out) {
    int rc = check_usable(c);
    if (rc) return rc;
    rc = check_groups_of(c, g, "nps_finish_groups_device");
    if (rc) return rc;
    if (!d_scores_out) return fail(NPS_E_INVAL, "d_scores_out is NULL");
    HIP_TRY(hipSetDevice(c->device));
    return finish_groups_common(c, g, offset, d_scores_out, nullptr, nloci_out);
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

// stats of the last resident run (nps_resident.hip) stay on the device until somebody asks for them
int materialize_resident_stats(nps_ctx *c) {
    if (!c->res_pending) return NPS_OK;
    // (a grouped run: G entries per row, group-minor -- a row without data repeats its one statistic for every group)
    const size_t G = c->groups ? (size_t)c->groups->n_groups : 1;
    const nps_locus_stat *src = c->groups ? c->d_grp_stats.get() : c->d_rstats.get();
    std::vector<nps_locus_stat> dev(c->res_m * G);
    if (c->res_m) {
        HIP_TRY(hipMemcpyAsync(dev.data(), src, sizeof(nps_locus_stat) * c->res_m * G,
                               hipMemcpyDeviceToHost, c->stream.get()));
        HIP_TRY(hipStreamSynchronize(c->stream.get()));
    }
    size_t h = 0;
    for (size_t j = 0; j < c->res_index.size(); ++j) {
        if (c->res_index[j] < 0) {
            c->ready.insert(c->ready.end(), G, c->res_host_stats[h++]);
            continue;
        }
        const nps_locus_stat *e = dev.data() + (size_t)c->res_index[j] * G;
        c->ready.insert(c->ready.end(), e, e + G);
    }
    c->res_pending = false;
    c->res_index.clear();
    c->res_host_stats.clear();
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
