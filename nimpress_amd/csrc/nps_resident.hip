// nps_resident.hip -- scoring a resident cohort (one of four units, nps_engine.h): the score definition nps_scoredef, the
// sample set nps_sampleset, the sample groups nps_samplegroups, and nps_score_cohort[_def[_subset | _groups]] with its three
// families of formats.  Host-side orchestration only; which fixed-point scales a definition gets is decided in nps_scale.h.
#include <cstdio>
#include <new>

#include "nps_engine.h"
#include "nps_group_labels.h"
#include "nps_scale.h"
#include "nps_subset_mask.h"

// ------------------------------------------------------------------------------------------
// score definitions kept on the device

// n row descriptors of the host, on the device
hipError_t upload_desc(DevBuf<nps_row_desc> &d, const nps_row_desc *rows, uint64_t n) {
    const hipError_t e = d.alloc(n);
    return e != hipSuccess ? e : hipMemcpy(d.get(), rows, sizeof(nps_row_desc) * n, hipMemcpyHostToDevice);
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
        // what the strip kernels make of the rows (nps_scale.h); below only the copies and uploads it asks for
        MxBandPlan plan = mx_band_plan(data.data(), d->m);
        d->special.swap(plan.special);
        d->mx_bound = plan.mx_bound;
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
        // rows are the definition's smallest): a copy of the fixed-point rows per band that costs a pass, beta = 0 outside
        // the band (every beta of `data` is finite by now)
        if (plan.used.size() > 1) {
            std::vector<nps_row_desc> copy(d->m);
            for (size_t u = 0; u < plan.used.size(); ++u) {
                nps_scoredef::MxBand mb;
                mb.bound = plan.used_bound[u];
                for (uint64_t j = 0; j < d->m; ++j) {
                    copy[j] = data[j];
                    if (plan.band[j] != plan.used[u]) copy[j].beta = 0.0;
                }
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
        r.F = mx_scale_exponent(bound);
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
// samples; the accumulation is the cohort's.  grp: a grouped run -- the three launches in their grouped form (nps_groups.hip),
// a tally and a decision per group, either dosage format)
static int score_run_ds(nps_ctx *c, RunGuard &guard, const nps_cohort *co, uint64_t cohort_row0, const nps_scoredef *def,
                        int mode, const FusedPlan &plan, uint64_t n_tally, const nps_sampleset *set,
                        const nps_samplegroups *grp = nullptr) {
    const uint64_t m = def->m;
    const uint64_t n_decide = set ? set->n_kept : c->n;
    const bool is_ds16 = co->format == NPS_FMT_DS16;
    const uint64_t stride_f = co->stride_bytes / 4;  // (NPS_FMT_DS32 only below the fused branch)
    const float *ds = (const float *)((const char *)co->d_data.get() + cohort_row0 * co->stride_bytes);
    if (plan.ok && c->n && !set && !grp) {
        bool ran = false;
        int rc = single_read(c, guard, plan, n_tally, "fused DS", mode == NPS_MODE_AUTO && !is_ds16, [&]() {
            return launch_ds_fused(c->stream.get(), plan, ds, co->stride_bytes, is_ds16 ? 2 : 4, c->n, m, def->d_desc.get(),
                                   dev_params(c->params), maxmis_threshold(c->n, c->params.max_missing_rate), c->d_rtally.get(),
                                   c->d_rstats.get(), c->d_nloci.get(), c->d_part_fused.get(), c->d_timeout.get());
        }, &ran);
        if (rc || ran) return rc;
    }
    if (is_ds16 && !grp) return fail(NPS_E_UNSUPPORTED, "NPS_FMT_DS16 cohorts are scored by the single-read kernel only");
    const int elem_bytes = is_ds16 ? 2 : 4;                   // (the grouped launches take rows of either format:
    const uint64_t stride_e = co->stride_bytes / elem_bytes;  //  their elements, and their stride in elements)
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
        if (grp) {
            const void *rows = (const char *)ds + r0 * co->stride_bytes;
            const int G = grp->n_groups;
            {
                ProfScope ps(c, P_TALLY);
                HIP_TRY(launch_groups_tally(c->stream.get(), rows, elem_bytes, stride_e, c->n, def->d_desc.get() + r0, k,
                                            grp->d_label.get(), grp->d_present.get(), G, c->d_grp_tally.get() + r0 * G));
            }
            {
                ProfScope ps(c, P_PARAMS);
                HIP_TRY(launch_groups_params(c->stream.get(), c->d_grp_tally.get() + r0 * G, def->d_desc.get() + r0, k, G,
                                             grp->d_size.get(), dev_params(c->params), c->d_grp_rowp.get() + r0,
                                             c->d_grp_imp.get() + r0 * 8, c->d_grp_stats.get() + r0 * G,
                                             c->d_nloci.get() + kGroupNloci));
            }
            {
                ProfScope ps(c, P_ACCUM);
                HIP_TRY(launch_groups_accumulate(c->stream.get(), rows, elem_bytes, stride_e, c->n, grp->d_label.get(),
                                                 c->d_grp_rowp.get() + r0, c->d_grp_imp.get() + r0 * 8, k, c->d_part.get(),
                                                 c->n_chunks, c->geom.part_chunk_stride));
            }
            continue;
        }
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

// a run's launches are queued: its rows without genotype data are applied, and its statistics wait for nps_flush
static void commit_run(nps_ctx *c, const nps_scoredef *def) {
    c->res_host_stats.clear();
    c->res_host_stats.reserve(def->host_rows.size());
    for (const nps_row_desc &r : def->host_rows) {  // host decided; nimpress.nim:526-558
        nps_locus_stat st;
        host_locus_row(c, r.kind, r.ref_is_effect, r.beta, r.eaf, &st);
        c->res_host_stats.push_back(st);
    }
    c->res_index = def->data_index;
    c->res_m = def->m;
    c->res_pending = true;
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
    if ((rc = check_ungrouped(c, set ? "nps_score_cohort_def_subset" : "nps_score_cohort_def"))) return rc;
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
        commit_run(c, def);
        c->plain_rows = true;
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
    if ((rc = check_ungrouped(c, "nps_score_cohort_def_subset"))) return rc;
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

// ------------------------------------------------------------------------------------------
// every group of a sample partition in one pass (the kernels: nps_groups.hip; the labels: nps_group_labels.h)
extern "C" int nps_samplegroups_create(nps_samplegroups **out, int device, uint64_t n_samples, const uint8_t *label, int n_groups) {
    if (!out) return fail(NPS_E_INVAL, "out is NULL");
    *out = nullptr;
    if (!label) return fail(NPS_E_INVAL, "label is NULL");
    if (n_samples == 0) return fail(NPS_E_INVAL, "sample groups of no samples");
    if (n_groups < 1 || n_groups > NPS_GROUPS_MAX) return fail(NPS_E_INVAL, "n_groups %d outside 1 .. %d", n_groups, NPS_GROUPS_MAX);
    if (n_samples > 0x7fffffffull) return fail(NPS_E_UNSUPPORTED, "n_samples %llu exceeds 2^31-1", (unsigned long long)n_samples);
    const GroupLabelCheck chk = group_labels_check(label, n_samples, n_groups);
    if (chk.error == kGroupLabelBad)
        return fail(NPS_E_INVAL, "sample %llu has label %d: neither a group 0 .. %d nor NPS_GROUP_NONE", (unsigned long long)chk.sample,
                    (int)label[chk.sample], n_groups - 1);
    if (chk.error == kGroupLabelsAllNone)
        return fail(NPS_E_INVAL, "every one of the %llu labels is NPS_GROUP_NONE: no sample in any group", (unsigned long long)n_samples);
    if (chk.error == kGroupLabelEmpty) return fail(NPS_E_INVAL, "group %d has no sample", chk.group);
    int rc = select_device(device);
    if (rc) return rc;
    const GroupLabels gl = group_labels(label, n_samples, n_groups);
    std::unique_ptr<nps_samplegroups> owner(new (std::nothrow) nps_samplegroups);
    nps_samplegroups *g = owner.get();
    if (!g) return fail(NPS_E_NOMEM, "out of host memory");
    g->device = device;
    g->n_samples = n_samples;
    g->n_groups = n_groups;
    unsigned long long size[kGroupsMax];
    for (int k = 0; k < kGroupsMax; ++k) size[k] = g->size[k] = gl.size[k];
    HIP_TRY(g->d_label.alloc(gl.label.size()));
    HIP_TRY(g->d_present.alloc(gl.present.size()));
    HIP_TRY(g->d_size.alloc(kGroupsMax));
    HIP_TRY(hipMemcpy(g->d_label.get(), gl.label.data(), gl.label.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(g->d_present.get(), gl.present.data(), gl.present.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(g->d_size.get(), size, sizeof size, hipMemcpyHostToDevice));
    *out = owner.release();
    return NPS_OK;
}
extern "C" int nps_samplegroups_n_groups(const nps_samplegroups *g) { return g ? g->n_groups : 0; }
extern "C" uint64_t nps_samplegroups_n_samples(const nps_samplegroups *g) { return g ? g->n_samples : 0; }
extern "C" uint64_t nps_samplegroups_size(const nps_samplegroups *g, int group) {
    return g && group >= 0 && group < g->n_groups ? g->size[group] : 0;
}
extern "C" void nps_samplegroups_destroy(nps_samplegroups *g) { delete g; }

// Everything is refused before the context changes, as for nps_score_cohort_def; the launches are score_run_ds's three per
// block of rows in their grouped form.  The context is grouped, with this groups object, once the first run is committed.
extern "C" int nps_score_cohort_def_groups(nps_ctx *c, const nps_cohort *co, uint64_t cohort_row0, const nps_scoredef *def,
                                           const nps_samplegroups *g) {
    int rc = check_usable(c);
    if (rc) return rc;
    if (!co || !def) return fail(NPS_E_INVAL, "cohort or scoredef is NULL");
    if (!g) return fail(NPS_E_INVAL, "groups is NULL");
    if (co->device != c->device || def->device != c->device)
        return fail(NPS_E_INVAL, "cohort / scoredef / context on different devices");
    if (g->device != c->device) return fail(NPS_E_INVAL, "sample groups and context are on different devices");
    if (g->n_samples != c->n)
        return fail(NPS_E_INVAL, "sample groups have %llu samples, context %llu", (unsigned long long)g->n_samples,
                    (unsigned long long)c->n);
    if (g->n_samples != co->n_samples)
        return fail(NPS_E_INVAL, "sample groups have %llu samples, cohort %llu", (unsigned long long)g->n_samples,
                    (unsigned long long)co->n_samples);
    if (co->format != NPS_FMT_DS32 && co->format != NPS_FMT_DS16)
        return fail(NPS_E_UNSUPPORTED, "sample groups are scored on NPS_FMT_DS32 and NPS_FMT_DS16 cohorts; this one is %s",
                    format_name(co->format));
    if (c->groups && c->groups != g)
        return fail(NPS_E_INVAL, "this context scores another groups object (one per context until nps_reset)");
    if (!c->groups && c->plain_rows)
        return fail(NPS_E_STATE, "a grouped call on a context that holds ungrouped rows; nps_reset first");
    const uint64_t m = def->m;
    rc = check_range(co, cohort_row0, m);
    if (rc) return rc;
    rc = cohort_quiesce(co);  // rows pushed into the cohort (nps_cohort_push_*) are complete
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    rc = materialize_resident_stats(c);  // (an earlier grouped run's entries leave d_grp_stats)
    if (rc) return rc;
    auto commit = [&]() {
        commit_run(c, def);
        c->groups = g;
    };
    if (m == 0) {
        commit();
        return NPS_OK;
    }
    // buffers (a failed allocation leaves the context usable: nothing has been queued yet)
    const uint64_t G = (uint64_t)g->n_groups;
    HIP_TRY(c->d_grp_tally.ensure(m * G, c->stream.get()));
    HIP_TRY(c->d_grp_rowp.ensure(m, c->stream.get()));
    HIP_TRY(c->d_grp_imp.ensure(m * 8, c->stream.get()));
    HIP_TRY(c->d_grp_stats.ensure(m * G, c->stream.get()));
    RunGuard guard{c};
    rc = score_run_ds(c, guard, co, cohort_row0, def, NPS_MODE_TWOPASS, FusedPlan{}, 0, nullptr, g);
    if (rc) return rc;
    commit();
    guard.ok = true;
    return NPS_OK;
}

extern "C" int nps_score_cohort(nps_ctx *c, const nps_cohort *co, uint64_t cohort_row0,
                                const nps_row_desc *rows, uint64_t n_desc, int mode) {
    if (!c || !co) return fail(NPS_E_INVAL, "ctx or cohort is NULL");
    if (int grc = check_ungrouped(c, "nps_score_cohort")) return grc;
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
