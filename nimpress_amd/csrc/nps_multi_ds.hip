// nps_multi_ds.hip -- several score definitions over a resident dosage cohort (NPS_FMT_DS32 / NPS_FMT_DS16) in TWO reads of
// the genotypes whatever the number of scores (reference loop nimpress.nim:634-641 run S times: S reads).
//
//   read 1  ds_tally_kernel<E, true> per cohort row: nmissing, sum DS and sum (2 - DS) over the non-missing samples -- the
//                                   tallies are the row's, not a score's: definitions may disagree about the effect allele
//           multi_ds_params_kernel  per (score, row): the decision chain of getImputedDosages (nps_row_decision.h) on the
//                                   sum the score's effect allele asks for -> one wave-uniform record
//   read 2  multi_ds_accumulate_kernel<S, E>   per lane four samples x S scores in float64, rows in order inside a row
//                                   chunk: score += dosage * beta (nim:639-641), exactly the operations of ds_accumulate_kernel
//           multi_ds_fold_kernel    the chunks' partial planes, in chunk order, into the context's running sums
//
// Plain IEEE float64 per lane: any finite dosage is taken (the [0, 2] range belongs to the fused single-score kernel),
// NaN imputed values and NaN constants need no flags, and the error is that of the single-score DS paths.  The library is
// built with -ffp-contract=off: the multiply and the add of a term stay two operations, as in the reference.
#include <algorithm>

#include "nps_ds_common.h"

namespace nps {

// one thread per (score = blockIdx.y, row).  ref_is_effect as in ds_params_kernel: == 1 flips the dosage (and takes the
// flipped sum), bit 0 alone selects the homref imputation value (NPS_RIE_COUNTS_EFFECT: the row counts the effect allele).
__global__ __launch_bounds__(256) void multi_ds_params_kernel(const MultiDsTally *__restrict__ tally,
                                                              const nps_row_desc *__restrict__ desc /* [S][n_desc] */,
                                                              uint64_t n_desc, int S, uint64_t n_samples, DevParams p,
                                                              DsRowP *__restrict__ rowp /* [n_desc][S] */,
                                                              MultiState *__restrict__ state) {
    const uint64_t row = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const int s = blockIdx.y;
    int used = 0;
    if (row < n_desc) {
        const nps_row_desc d = desc[(uint64_t)s * n_desc + row];
        const bool rie = (d.ref_is_effect & 1) != 0;
        const bool flip = d.ref_is_effect == 1;
        RowDecision dec{0, 0, 0, 0.0};  // NPS_ROW_NOT_IN_SCORE: the row is not part of this score
        if (d.kind == NPS_ROW_PRESENT) {
            const MultiDsTally t = tally[row];
            const uint64_t nmiss = t.nmiss, ngen = n_samples - nmiss;
            dec = decide_row(p, over_maxmis(nmiss, n_samples, p.max_missing_rate), d.eaf, rie, flip ? t.sum_flipped : t.sum,
                             ngen);
        } else if (d.kind == NPS_ROW_ABSENT || d.kind == NPS_ROW_UNCOVERED || d.kind == NPS_ROW_FILTERED) {
            dec = no_data_row(p, d.kind, d.eaf, rie);
        }
        used = dec.used;
        // (mode 0 adds 0 x 0: multi_ds_accumulate_kernel has no branch)
        rowp[row * (uint64_t)S + s] = ds_row_record(dec, dec.mode ? d.beta : 0.0, flip);
    }
    const int cnt = __syncthreads_count(used);
    if (threadIdx.x == 0 && cnt) atomicAdd(&state[s].nloci, (unsigned long long)cnt);
}

// The hot path, modelled on ds_accumulate_kernel: a lane owns FOUR neighbouring samples and 4 S float64 accumulators; per
// row one non-temporal load (16 bytes of float32, 8 of DS16; the rows are read once here and are zero padded to 64
// elements, so the load of a row's last lanes stays inside it), eight rows in flight, rows in order.  Per genotype the
// conversion and 2 - DS are formed once; per score the term is a select and d * beta, then the add.  The S records of a
// row are the same for every lane: their address depends on the row alone, and the compiler reads them into scalar
// registers (s_load) -- the selects between the record's values are scalar too.
// grid.y row chunks write partial planes [chunk][score][plane_stride]; the pad lanes of a plane's last four are written
// too (from the row's zero padding) and never read.
template <int S, typename E>
__global__ __launch_bounds__(256) void multi_ds_accumulate_kernel(const E *__restrict__ ds, uint64_t stride_e, uint64_t n,
                                                                  const DsRowP *__restrict__ rowp_all, uint64_t n_rows_all,
                                                                  uint64_t rows_per_chunk, double *__restrict__ planes,
                                                                  uint64_t plane_stride) {
    typedef typename DsElem<E>::v4 V4;
    const uint64_t i = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    const uint64_t r_begin = (uint64_t)blockIdx.y * rows_per_chunk;
    if (i >= n || r_begin >= n_rows_all) return;
    const uint64_t n_rows = min(rows_per_chunk, n_rows_all - r_begin);
    const DsRowP *rowp = rowp_all + r_begin * S;
    double acc[S][4];
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[s][k] = 0.0;
    const E *p = ds + r_begin * stride_e + i;
    auto apply = [&](uint64_t row, const V4 q) {
        double dp[4], df[4];
        uint64_t nan[4];  // the wave's lanes whose sample k is missing
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float e = DsElem<E>::value(q[k]);
            nan[k] = __builtin_amdgcn_ballot_w64(isnan(e));
            dp[k] = (double)e;
            df[k] = 2.0 - dp[k];
        }
        // the row's S records first, then the arithmetic: no branch, one wait for the scalar loads of a row
        DsRowP r[S];
#pragma unroll
        for (int s = 0; s < S; ++s) r[s] = rowp[row * S + s];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            // mode 1: the row's dosages, imp for a missing sample; mode 2: cst for every sample; mode 0: the params kernel
            // wrote beta = cst = 0, every sample adds 0 x 0 (the running sums never hold -0, so adding +0 changes nothing)
            const bool all = r[s].mode != 1;
            const uint64_t all_lanes = all ? ~0ull : 0ull;
            const double masked = all ? r[s].cst : r[s].imp;
            const bool flip = r[s].rie != 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double dv = flip ? df[k] : dp[k];
                // (lane masks ORed as scalars: one select per half of the double, not two)
                const double d = __builtin_amdgcn_inverse_ballot_w64(nan[k] | all_lanes) ? masked : dv;
                acc[s][k] += d * r[s].beta;
            }
        }
    };
    auto load = [&](uint64_t row) { return __builtin_nontemporal_load(reinterpret_cast<const V4 *>(p + row * stride_e)); };
    uint64_t row = 0;
    for (; row + 8 <= n_rows; row += 8) {
        V4 q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) q[u] = load(row + u);
#pragma unroll
        for (int u = 0; u < 8; ++u) apply(row + u, q[u]);
    }
    for (; row < n_rows; ++row) apply(row, load(row));
    double *dst = planes + (uint64_t)blockIdx.y * S * plane_stride + i;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        double2 *o = reinterpret_cast<double2 *>(dst + (uint64_t)s * plane_stride);
        o[0] = make_double2(acc[s][0], acc[s][1]);
        o[1] = make_double2(acc[s][2], acc[s][3]);
    }
}

// one thread per (sample, score = blockIdx.y): the chunks in order, then into the running sum
__global__ __launch_bounds__(256) void multi_ds_fold_kernel(const double *__restrict__ planes, uint32_t n_chunks, int S,
                                                            uint64_t plane_stride, uint64_t n, double *__restrict__ part,
                                                            int overwrite) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const int s = blockIdx.y;
    if (i >= n) return;
    const double *src = planes + (uint64_t)s * plane_stride + i;
    double v = src[0];
    for (uint32_t c = 1; c < n_chunks; ++c) v += src[(uint64_t)c * S * plane_stride];
    double *dst = part + (uint64_t)s * n + i;
    *dst = overwrite ? v : *dst + v;
}

// ---- host side ------------------------------------------------------------------------------
MultiDsPlan multi_ds_plan(uint64_t n_samples, uint64_t n_rows, int cus) {
    MultiDsPlan pl;
    pl.plane_stride = (std::max<uint64_t>(n_samples, 1) + 3) / 4 * 4;
    if (n_rows == 0) return pl;
    // eight workgroups of four waves per compute unit fill the chip at this kernel's register count; a workgroup covers
    // 1 024 samples, the row chunks make up the rest -- each at least 16 rows long (two turns of the eight-row loop)
    const uint64_t bx = std::max<uint64_t>(1, (n_samples + 1023) / 1024);
    const uint64_t want = std::max<uint64_t>(1, ((uint64_t)std::max(cus, 1) * 8 + bx - 1) / bx);
    uint64_t rpc = std::max<uint64_t>(16, (n_rows + want - 1) / want);
    rpc = std::max<uint64_t>(rpc, (n_rows + 65534) / 65535);  // (grid.y)
    pl.rows_per_chunk = rpc;
    pl.n_chunks = (uint32_t)((n_rows + rpc - 1) / rpc);
    return pl;
}

hipError_t launch_multi_ds_tally(hipStream_t st, const void *d_ds, int elem_bytes, uint64_t stride_e, uint64_t n,
                                 uint64_t n_rows, MultiDsTally *d_tally) {
    if (n_rows == 0) return hipSuccess;
    if (n_rows > 0x7fffffffull || (elem_bytes != 2 && elem_bytes != 4)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    // ds_tally_kernel (nps_ds_common.h) with both sums side by side: they have the bits of the neffect the single-score
    // paths give the row with ref_is_effect 0 and 1, because they come from the same kernel text
    const dim3 grid((uint32_t)n_rows), block(256);
    if (elem_bytes == 4)
        hipLaunchKernelGGL((ds_tally_kernel<float, true>), grid, block, 0, st, (const float *)d_ds, stride_e, n, nullptr, n_rows,
                           d_tally);
    else
        hipLaunchKernelGGL((ds_tally_kernel<uint16_t, true>), grid, block, 0, st, (const uint16_t *)d_ds, stride_e, n, nullptr,
                           n_rows, d_tally);
    return hipGetLastError();
}

hipError_t launch_multi_ds_params(hipStream_t st, const MultiDsTally *d_tally, const nps_row_desc *d_desc, uint64_t n_desc,
                                  int S, uint64_t n_samples, DevParams p, DsRowP *d_rowp, void *d_state) {
    if (n_desc == 0 || S == 0) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(multi_ds_params_kernel, dim3((uint32_t)((n_desc + 255) / 256), (uint32_t)S), dim3(256), 0, st, d_tally,
                       d_desc, n_desc, S, n_samples, p, d_rowp, (MultiState *)d_state);
    return hipGetLastError();
}

template <int S, typename E>
static void launch_mds_accumulate_s(hipStream_t st, const MultiDsPlan &pl, const void *d_ds, uint64_t stride_e, uint64_t n,
                                    const DsRowP *d_rowp, uint64_t n_rows, double *d_planes) {
    hipLaunchKernelGGL((multi_ds_accumulate_kernel<S, E>), dim3((uint32_t)((n + 1023) / 1024), pl.n_chunks), dim3(256), 0, st,
                       (const E *)d_ds, stride_e, n, d_rowp, n_rows, pl.rows_per_chunk, d_planes, pl.plane_stride);
}

template <typename E>
static hipError_t launch_mds_accumulate_e(hipStream_t st, const MultiDsPlan &pl, const void *d_ds, uint64_t stride_e,
                                          uint64_t n, const DsRowP *d_rowp, uint64_t n_rows, int S, double *d_planes) {
    switch (S) {
    case 1: launch_mds_accumulate_s<1, E>(st, pl, d_ds, stride_e, n, d_rowp, n_rows, d_planes); break;
    case 2: launch_mds_accumulate_s<2, E>(st, pl, d_ds, stride_e, n, d_rowp, n_rows, d_planes); break;
    case 3: launch_mds_accumulate_s<3, E>(st, pl, d_ds, stride_e, n, d_rowp, n_rows, d_planes); break;
    case 4: launch_mds_accumulate_s<4, E>(st, pl, d_ds, stride_e, n, d_rowp, n_rows, d_planes); break;
    case 5: launch_mds_accumulate_s<5, E>(st, pl, d_ds, stride_e, n, d_rowp, n_rows, d_planes); break;
    case 6: launch_mds_accumulate_s<6, E>(st, pl, d_ds, stride_e, n, d_rowp, n_rows, d_planes); break;
    case 7: launch_mds_accumulate_s<7, E>(st, pl, d_ds, stride_e, n, d_rowp, n_rows, d_planes); break;
    case 8: launch_mds_accumulate_s<8, E>(st, pl, d_ds, stride_e, n, d_rowp, n_rows, d_planes); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_multi_ds_accumulate(hipStream_t st, const MultiDsPlan &pl, const void *d_ds, int elem_bytes, uint64_t stride_e,
                                      uint64_t n, const DsRowP *d_rowp, uint64_t n_rows, int S, double *d_planes) {
    if (n_rows == 0 || n == 0) return hipSuccess;
    if (pl.n_chunks == 0 || pl.n_chunks > 65535 || pl.plane_stride < n || (uint64_t)pl.n_chunks * pl.rows_per_chunk < n_rows ||
        (elem_bytes != 2 && elem_bytes != 4))
        return hipErrorInvalidValue;
    (void)hipGetLastError();
    return elem_bytes == 4 ? launch_mds_accumulate_e<float>(st, pl, d_ds, stride_e, n, d_rowp, n_rows, S, d_planes)
                           : launch_mds_accumulate_e<uint16_t>(st, pl, d_ds, stride_e, n, d_rowp, n_rows, S, d_planes);
}

hipError_t launch_multi_ds_fold(hipStream_t st, const MultiDsPlan &pl, const double *d_planes, uint64_t n, int S, double *d_part,
                                int overwrite) {
    if (n == 0 || pl.n_chunks == 0) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(multi_ds_fold_kernel, dim3((uint32_t)((n + 255) / 256), (uint32_t)S), dim3(256), 0, st, d_planes,
                       pl.n_chunks, S, pl.plane_stride, n, d_part, overwrite);
    return hipGetLastError();
}

}  // namespace nps
