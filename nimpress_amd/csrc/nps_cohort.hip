// nps_cohort.hip -- the resident cohort nps_cohort of include/nps.h (one of four units, nps_engine.h): create, optimize,
// upload / download / upload_bed, rows pushed and decoded on the device, the synthetic generator, convert, and the
// whole-row tallies a strip cohort keeps.  Host-side orchestration only: the kernels are in nps_kernels.hip, nps_mx.hip
// and nps_pl.hip.
#include <new>

#include "nps_engine.h"

// ---- NPS_FMT_GT2X: which superblocks carry their tally words ------------------------------------------------------
bool mx_tallies_valid(const nps_cohort *c, uint64_t sb0, uint64_t n_sb) {
    if (!c->mx_sb_valid) return n_sb == 0;
    if (n_sb == gt2x_superblocks(c->n_rows)) return c->mx_sb_valid_count.load(std::memory_order_acquire) == n_sb;
    for (uint64_t sb = sb0; sb < sb0 + n_sb; ++sb)
        if (!((c->mx_sb_valid[sb >> 6].load(std::memory_order_acquire) >> (sb & 63)) & 1ull)) return false;
    return true;
}
static bool mx_tallies_all_valid(const nps_cohort *c) { return mx_tallies_valid(c, 0, gt2x_superblocks(c->n_rows)); }
// tally_mutex held.  valid = true only once the words of these superblocks ARE in device memory.
void mx_tallies_mark(nps_cohort *c, uint64_t sb0, uint64_t n_sb, bool valid) {
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
hipError_t mx_tallies_alloc(nps_cohort *c) {
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

// rows pushed into the cohort (nps_cohort_push_*) are complete
int cohort_quiesce(const nps_cohort *c) {
    if (c && c->push_stream.get()) HIP_TRY(hipStreamSynchronize(c->push_stream.get()));
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

int check_range(const nps_cohort *c, uint64_t row0, uint64_t nrows) {
    if (!c) return fail(NPS_E_INVAL, "cohort is NULL");
    if (row0 > c->n_rows || nrows > c->n_rows - row0)
        return fail(NPS_E_INVAL, "rows [%llu,+%llu) outside cohort of %llu rows",
                    (unsigned long long)row0, (unsigned long long)nrows,
                    (unsigned long long)c->n_rows);
    return NPS_OK;
}

// the group-interleaved device layout -> GT2 rows, through a host buffer of whole groups (uploads: gt2_upload)
static int gt2_download(const nps_cohort *c, uint64_t row0, uint64_t nrows, void *host_rows, size_t host_stride) {
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
        HIP_TRY(hipMemcpy(buf.data(), dev, groups * sw * 16, hipMemcpyDeviceToHost));
        if (c->optimized)  // parity layout -> plain, on the copy
            for (uint64_t x = 0; x < groups * sw; ++x) {
                uint32_t *q = buf.data() + x * 4;
                q[0] = parity_fix(q[0], q[1], q[2], q[3]);
            }
        for (uint64_t j = 0; j < k; ++j) {
            uint32_t *hrow = (uint32_t *)((char *)host_rows + (r + j) * host_stride);
            const uint32_t *g = buf.data() + (j >> 2) * sw * 4 + (j & 3);
            for (uint64_t w = 0; w < n_words; ++w) hrow[w] = word_from_planes(g[w * 4]);
        }
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
    if (c->format == NPS_FMT_GT2) return gt2_download(c, row0, nrows, host_rows, host_stride);
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
// the unit layouts from a NPS_FMT_GT2 cohort: NPS_FMT_GT2M (the multi-score pass, nps_multi.hip) and NPS_FMT_GT2X (the strips)
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
int mx_keep_tallies_locked(nps_cohort *c) {
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
