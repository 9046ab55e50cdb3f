// nps_multiscore.hip -- several score definitions in one pass (one of four units, nps_engine.h): the definitions
// nps_multidef and the context nps_multi, over a NPS_FMT_GT2M cohort (one read, nps_multi.hip) or a dosage cohort (two
// reads, nps_multi_ds.hip).  Host-side orchestration only; the fixed-point scale of every score is decided in nps_scale.h.
#include <new>

#include "nps_engine.h"
#include "nps_scale.h"

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
    // one fixed-point scale per score, or the first refusal (nps_scale.h) -- before a device is touched
    const MultiScale sc = multi_scale(rows, n_scores, n_desc, ND);
    const int s = sc.score;
    const unsigned long long j = sc.row;
    switch (sc.refusal) {
    case MultiScale::None: break;
    case MultiScale::BadKind:
        return fail(NPS_E_INVAL, "score %d row %llu: bad kind %d", s, j, rows[(uint64_t)s * n_desc + j].kind);
    case MultiScale::BetaNotFinite:
        return fail(NPS_E_UNSUPPORTED, "score %d row %llu: beta is not finite (use the single-score path)", s, j);
    case MultiScale::EafInfinite:
        return fail(NPS_E_UNSUPPORTED, "score %d row %llu: eaf is infinite (use the single-score path)", s, j);
    case MultiScale::Span:
        return fail(NPS_E_UNSUPPORTED, "score %d: |beta| spans %.3g (%.3g .. %.3g), more than the 2^%d one %d-bit "
                    "fixed-point scale holds within 1e-6 relative; score this definition with the single-score path "
                    "(nps_scoredef_create / nps_score_cohort_def: magnitude bands), the others in one pass",
                    s, sc.maxb / sc.minb, sc.minb, sc.maxb, multi_span_bits(ND), 8 * ND - 7);
    }
    int rc = select_device(device);
    if (rc) return rc;
    std::unique_ptr<nps_multidef> owner(new (std::nothrow) nps_multidef);
    nps_multidef *d = owner.get();
    if (!d) return fail(NPS_E_NOMEM, "out of host memory");
    d->device = device;
    d->S = n_scores;
    d->ND = ND;
    d->no_scale = sc.no_scale;
    d->n_desc = n_desc;
    HIP_TRY(d->d_F.alloc(NPS_MULTI_MAX_SCORES));
    HIP_TRY(hipMemcpy(d->d_F.get(), sc.F, sizeof(int) * n_scores, hipMemcpyHostToDevice));
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

// what check_usable is to nps_ctx
static int multi_usable(const nps_multi *m) {
    if (!m) return fail(NPS_E_INVAL, "ctx is NULL");
    if (m->broken) return fail(NPS_E_STATE, "an earlier pass failed on the device: nps_multi_reset first");
    return NPS_OK;
}

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
    if (int urc = multi_usable(m)) return urc;
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
    if (int urc = multi_usable(m)) return urc;
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
    if (int urc = multi_usable(m)) return urc;
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
