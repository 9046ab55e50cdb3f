// nps_groups.hip -- every group of a sample partition in one pass over a dosage cohort (nps_score_cohort_def_groups,
// include/nps.h): the grouped forms of the three launches of the two-pass dosage route (nps_ds.hip) and of the finish.
//
//   read 1  groups_tally_kernel<E, G>      per row one (nmissing, sum of dosages) pair per group
//           groups_params_kernel           per (row, group) the row's decision; per row one record for the accumulation
//   read 2  groups_accumulate_kernel<E>    per sample its own group's decision: s += d * beta, rows in order
//           groups_finish_kernel           nimpress.nim:643-649 with the nloci of the sample's group
//
// Plain streaming kernels: no cooperative launch, no wait of one workgroup for another.  What the run promises in bits:
// group k's tallies are those of ds_tally_masked_kernel under the mask {label == k}, a sample's sum is that of
// ds_accumulate_kernel with its group's decisions -- so G groups here are G subset runs, bit for bit, in two reads.
// E: float (NPS_FMT_DS32) or uint16_t (NPS_FMT_DS16), through DsElem<E>; the labels: nps_group_labels.h.
#include <algorithm>

#include "nps_ds_common.h"

namespace nps {

// THE SUMMATION TREE of ds_tally_kernel (nps_ds_common.h), kept once per group: the same lanes-of-four in the same order,
// the same wave and block combine.  A thread adds the term of a sample to EVERY group's sum that occurs in the sample's
// block, as `label == k ? value : +0.0`: a sum starts at +0.0 and can never become -0.0 (+0.0 + -0.0 = +0.0 under round to
// nearest), and x + (+0.0) has the bits of x for every other x -- so group k's sum has the bits it has when only its own
// samples are added, which is what ds_tally_masked_kernel does.  Missing samples count and never enter a sum.
// label4: the four labels of lane-of-four v in one word (padding samples: 255, no group); present: one byte per block of
// 256 samples = per wave and load, bit k set when group k occurs there -- a wave-uniform value (readfirstlane: the branches
// on it are scalar).  A block without a grouped sample is not read, a group that does not occur in it is not added to: a
// cohort sorted by group costs what one group costs.  The sums and counts are arrays indexed by unrolled loops only
// (registers, never scratch).  G: the groups rounded up to 2, 4 or 8; the bits do not depend on it.
template <typename E, int G>
__global__ __launch_bounds__(256) void groups_tally_kernel(const E *__restrict__ ds, uint64_t stride_e, uint64_t n,
                                                           const nps_row_desc *__restrict__ desc, uint64_t n_rows,
                                                           const uint32_t *__restrict__ label4,
                                                           const unsigned char *__restrict__ present, int n_groups,
                                                           DsTally *__restrict__ out /* [n_rows][n_groups] */) {
    typedef typename DsElem<E>::v4 V4;
    __shared__ double s_sum[G][4];
    __shared__ uint32_t s_cnt[G][4];
    const uint64_t row = blockIdx.x;
    if (row >= n_rows) return;
    const bool rie = desc[row].ref_is_effect == 1;  // bit 1 set: the row already counts the effect allele
    const V4 *p = reinterpret_cast<const V4 *>(ds + row * stride_e);
    const uint64_t n4 = (n + 3) / 4;  // rows are zero padded to a multiple of 64 elements, the labels with 255
    uint32_t cnt[G];
    double sum[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        cnt[g] = 0;
        sum[g] = 0.0;
    }
    auto occurs = [&](uint64_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)present[v >> 6]); };
    auto take = [&](const V4 q, uint32_t lab, uint32_t pres) {
        if (pres == 0) return;
        double d[4];
        uint32_t lv[4], lm[4];  // the group whose sum takes the value / whose count takes the sample (256: nobody's)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float e = DsElem<E>::value(q[k]);
            const uint32_t l = (lab >> (8 * k)) & 255u;
            const bool miss = isnan(e);
            d[k] = rie ? 2.0 - (double)e : (double)e;
            lv[k] = miss ? 256u : l;
            lm[k] = miss ? l : 256u;
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (pres & (1u << g)) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    sum[g] += lv[k] == (uint32_t)g ? d[k] : 0.0;
                    cnt[g] += lm[k] == (uint32_t)g ? 1u : 0u;
                }
            }
        }
    };
    uint64_t v = threadIdx.x;
    for (; v + 7 * 256 < n4; v += 8 * 256) {
        V4 q[8];
        uint32_t lab[8], pres[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) pres[u] = occurs(v + u * 256);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            q[u] = V4{0, 0, 0, 0};
            lab[u] = 0xffffffffu;
            if (pres[u]) {
                q[u] = p[v + u * 256];
                lab[u] = label4[v + u * 256];
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) take(q[u], lab[u], pres[u]);
    }
    for (; v < n4; v += 256) {
        const uint32_t pres = occurs(v);
        if (pres) take(p[v], label4[v], pres);
    }
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (g < n_groups) {
            const double s = wave_sum_f64(sum[g]);
            const uint32_t c = wave_sum_u32(cnt[g]);
            if ((threadIdx.x & 63) == 0) {
                s_sum[g][w] = s;
                s_cnt[g][w] = c;
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < n_groups) {
        const int g = threadIdx.x;
        DsTally t;
        t.nmiss = (unsigned long long)s_cnt[g][0] + s_cnt[g][1] + s_cnt[g][2] + s_cnt[g][3];
        t.neff = ((s_sum[g][0] + s_sum[g][1]) + s_sum[g][2]) + s_sum[g][3];
        out[row * (uint64_t)n_groups + g] = t;
    }
}

// one thread per (row, group): 32 rows x 8 group slots per block, a row's slots in neighbouring lanes.  The decision is
// ds_params_kernel's with N = the group's size; the 2-bit modes of a row's groups are ORed into one word across the
// row's eight lanes, slot 0 writes the row's record.  nloci: the integer idiom of ds_params_kernel, once per group.
__global__ __launch_bounds__(256) void groups_params_kernel(const DsTally *__restrict__ tally /* [n_rows][n_groups] */,
                                                            const nps_row_desc *__restrict__ desc, uint64_t n_rows,
                                                            int n_groups, const unsigned long long *__restrict__ size,
                                                            DevParams p, GroupRowP *__restrict__ rowp,
                                                            double *__restrict__ imp /* [n_rows][8] */,
                                                            nps_locus_stat *__restrict__ stats /* [n_rows][n_groups] */,
                                                            unsigned long long *__restrict__ nloci /* [8] */) {
    const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t row = idx >> 3;
    const int k = (int)(idx & 7);
    int used = 0;
    uint32_t modes = 0;
    if (row < n_rows && k < n_groups) {
        const DsTally t = tally[row * (uint64_t)n_groups + k];
        const uint64_t nmiss = t.nmiss, n_k = size[k], ngen = n_k - nmiss;
        const bool rie = (desc[row].ref_is_effect & 1) != 0;  // homref imputation value
        const RowDecision d = decide_row(p, over_maxmis(nmiss, n_k, p.max_missing_rate), desc[row].eaf, rie, t.neff, ngen);
        used = d.used;
        modes = (uint32_t)d.mode << (2 * k);
        imp[row * 8 + k] = d.mode == 1 ? d.imp : 0.0;
        stats[row * (uint64_t)n_groups + k] = row_stat(d, ngen, nmiss, t.neff);
    }
    modes |= __shfl_xor(modes, 1, 64);
    modes |= __shfl_xor(modes, 2, 64);
    modes |= __shfl_xor(modes, 4, 64);
    if (row < n_rows && k == 0) {
        GroupRowP r;
        r.beta = desc[row].beta;
        // the constant of a row over --maxmis is the row's alone (imputeLocusDosages, nimpress.nim:417-447)
        (void)locus_dosage(p, desc[row].eaf, (desc[row].ref_is_effect & 1) != 0, r.cst);
        r.modes = modes;
        r.rie = desc[row].ref_is_effect == 1 ? 1 : 0;  // dosage = 2 - DS
        rowp[row] = r;
    }
    for (int g = 0; g < n_groups; ++g) {
        const int cnt = __syncthreads_count(used && k == g);
        if (threadIdx.x == 0 && cnt) atomicAdd(nloci + g, (unsigned long long)cnt);
    }
}

// ds_accumulate_kernel (nps_ds.hip) with a decision per sample: the same grid, chunks and partial planes, one thread = FOUR
// neighbouring samples x one chunk of rows, rows in order, one non-temporal load per row and thread, eight in flight.  The
// thread's four labels stay in registers as shifts into the row's mode word (a sample without a group shifts to the
// word's empty bits: mode 0).  The record is the same for every lane (scalar loads); the imputation value of a sample's
// group is fetched per lane, and only where a lane of the wave has a missing sample in a genotyped row.  Per sample and
// row exactly that kernel's `s += d * beta`; a mode-0 row is skipped for the sample, not multiplied by zero.
template <typename E>
__global__ __launch_bounds__(256) void groups_accumulate_kernel(const E *__restrict__ ds, uint64_t stride_e, uint64_t n,
                                                                const uint32_t *__restrict__ label4,
                                                                const GroupRowP *__restrict__ rowp_all,
                                                                const double *__restrict__ imp_all, uint64_t n_rows_all,
                                                                uint64_t rows_per_chunk, double *__restrict__ part,
                                                                uint64_t part_chunk_stride) {
    typedef typename DsElem<E>::v4 V4;
    const uint64_t i = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    const uint64_t r_begin = (uint64_t)blockIdx.y * rows_per_chunk;
    if (i >= n || r_begin >= n_rows_all) return;
    const uint64_t n_rows = min(rows_per_chunk, n_rows_all - r_begin);
    const GroupRowP *rowp = rowp_all + r_begin;
    const double *imp = imp_all + r_begin * 8;
    double *part0 = part + (uint64_t)blockIdx.y * part_chunk_stride + i;
    const int live = (int)min((uint64_t)4, n - i);
    const uint32_t lab = label4[i >> 2];
    uint32_t sh[4], gi[4];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t l = (lab >> (8 * k)) & 255u;
        sh[k] = l < 8u ? 2u * l : 16u;  // (bits 16, 17 of the mode word are never set)
        gi[k] = l & 7u;
        if (k < live) s[k] = part0[k];
    }
    const E *p = ds + r_begin * stride_e + i;
    auto apply = [&](uint64_t row, const V4 q) {
        const GroupRowP r = rowp[row];
        if (r.modes == 0) return;
        float e[4];
        uint32_t m[4];
        bool miss[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            e[k] = DsElem<E>::value(q[k]);
            m[k] = (r.modes >> sh[k]) & 3u;
            miss[k] = m[k] == 1u && isnan(e[k]);
        }
        double iv[4] = {0.0, 0.0, 0.0, 0.0};
        if (__any(miss[0] || miss[1] || miss[2] || miss[3])) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (miss[k]) iv[k] = imp[row * 8 + gi[k]];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (m[k] != 0u) {
                double d;
                if (m[k] == 2u)
                    d = r.cst;
                else if (miss[k])
                    d = iv[k];
                else
                    d = r.rie ? 2.0 - (double)e[k] : (double)e[k];
                s[k] += d * r.beta;
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
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < live) part0[k] = s[k];
}

// finish_kernel (nps_kernels.hip) with the nloci of the sample's group: the chunk planes in the same order, const_sum added
// the same way; a sample without a group gets the NaN of row_nan()
__global__ __launch_bounds__(256) void groups_finish_kernel(const double *__restrict__ part, uint32_t n_chunks,
                                                            uint64_t part_chunk_stride, uint64_t n_samples, double const_sum,
                                                            const unsigned char *__restrict__ label,
                                                            const unsigned long long *__restrict__ d_nloci /* [8] */,
                                                            uint64_t host_nloci, double offset, double *__restrict__ scores) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_samples) return;
    const uint32_t l = label[i];
    if (l >= 8u) {
        scores[i] = row_nan();
        return;
    }
    double s = 0.0;
    for (uint32_t c = 0; c < n_chunks; ++c) s += part[(uint64_t)c * part_chunk_stride + i];
    s += const_sum;
    const uint64_t nloci = host_nloci + (uint64_t)d_nloci[l];
    s /= (double)nloci * 2.0;  // nimpress.nim:645 (nloci = 0: 0/0 = NaN, as in the reference)
    s += offset;               // nimpress.nim:649
    scores[i] = s;
}

// ---- launchers --------------------------------------------------------------------------------
template <typename E>
static hipError_t launch_groups_tally_e(hipStream_t st, const void *d_ds, uint64_t stride_e, uint64_t n,
                                        const nps_row_desc *d_desc, uint64_t n_rows, const unsigned char *d_label,
                                        const unsigned char *d_present, int n_groups, DsTally *d_tally) {
    const dim3 grid((uint32_t)n_rows), block(256);
    const E *ds = (const E *)d_ds;
    const uint32_t *label4 = (const uint32_t *)d_label;
    if (n_groups <= 2)
        hipLaunchKernelGGL((groups_tally_kernel<E, 2>), grid, block, 0, st, ds, stride_e, n, d_desc, n_rows, label4, d_present,
                           n_groups, d_tally);
    else if (n_groups <= 4)
        hipLaunchKernelGGL((groups_tally_kernel<E, 4>), grid, block, 0, st, ds, stride_e, n, d_desc, n_rows, label4, d_present,
                           n_groups, d_tally);
    else
        hipLaunchKernelGGL((groups_tally_kernel<E, 8>), grid, block, 0, st, ds, stride_e, n, d_desc, n_rows, label4, d_present,
                           n_groups, d_tally);
    return hipGetLastError();
}

hipError_t launch_groups_tally(hipStream_t st, const void *d_ds, int elem_bytes, uint64_t stride_e, uint64_t n,
                               const nps_row_desc *d_desc, uint64_t n_rows, const unsigned char *d_label,
                               const unsigned char *d_present, int n_groups, DsTally *d_tally) {
    if (n_rows == 0) return hipSuccess;
    if (n_rows > 0x7fffffffull || n_groups < 1 || n_groups > 8 || (elem_bytes != 2 && elem_bytes != 4)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    return elem_bytes == 4 ? launch_groups_tally_e<float>(st, d_ds, stride_e, n, d_desc, n_rows, d_label, d_present, n_groups, d_tally)
                           : launch_groups_tally_e<uint16_t>(st, d_ds, stride_e, n, d_desc, n_rows, d_label, d_present, n_groups,
                                                             d_tally);
}

hipError_t launch_groups_params(hipStream_t st, const DsTally *d_tally, const nps_row_desc *d_desc, uint64_t n_rows, int n_groups,
                                const unsigned long long *d_size, DevParams p, GroupRowP *d_rowp, double *d_imp,
                                nps_locus_stat *d_stats, unsigned long long *d_nloci) {
    if (n_rows == 0) return hipSuccess;
    if (n_groups < 1 || n_groups > 8 || n_rows > (0x7fffffffull << 5)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(groups_params_kernel, dim3((uint32_t)((n_rows + 31) / 32)), dim3(256), 0, st, d_tally, d_desc, n_rows,
                       n_groups, d_size, p, d_rowp, d_imp, d_stats, d_nloci);
    return hipGetLastError();
}

hipError_t launch_groups_accumulate(hipStream_t st, const void *d_ds, int elem_bytes, uint64_t stride_e, uint64_t n,
                                    const unsigned char *d_label, const GroupRowP *d_rowp, const double *d_imp, uint64_t n_rows,
                                    double *d_part, uint32_t n_chunks, uint64_t part_chunk_stride) {
    if (n_rows == 0 || n == 0) return hipSuccess;
    if (n_chunks == 0 || n_chunks > 65535 || part_chunk_stride < n || (elem_bytes != 2 && elem_bytes != 4))
        return hipErrorInvalidValue;
    const uint64_t rows_per_chunk = std::max<uint64_t>(16, (n_rows + n_chunks - 1) / n_chunks);
    const dim3 grid((uint32_t)((n + 1023) / 1024), n_chunks), block(256);
    const uint32_t *label4 = (const uint32_t *)d_label;
    (void)hipGetLastError();
    if (elem_bytes == 4)
        hipLaunchKernelGGL(groups_accumulate_kernel<float>, grid, block, 0, st, (const float *)d_ds, stride_e, n, label4, d_rowp,
                           d_imp, n_rows, rows_per_chunk, d_part, part_chunk_stride);
    else
        hipLaunchKernelGGL(groups_accumulate_kernel<uint16_t>, grid, block, 0, st, (const uint16_t *)d_ds, stride_e, n, label4,
                           d_rowp, d_imp, n_rows, rows_per_chunk, d_part, part_chunk_stride);
    return hipGetLastError();
}

hipError_t launch_groups_finish(hipStream_t st, const double *d_part, uint32_t n_chunks, uint64_t part_chunk_stride,
                                uint64_t n_samples, double const_sum, const unsigned char *d_label,
                                const unsigned long long *d_nloci, uint64_t host_nloci, double offset, double *d_scores) {
    if (n_samples == 0) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(groups_finish_kernel, dim3((uint32_t)((n_samples + 255) / 256)), dim3(256), 0, st, d_part, n_chunks,
                       part_chunk_stride, n_samples, const_sum, d_label, d_nloci, host_nloci, offset, d_scores);
    return hipGetLastError();
}

}  // namespace nps
