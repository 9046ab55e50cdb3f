// nps_subset.hip -- scoring a chosen subset of a resident cohort's samples (nps_score_cohort_def_subset, include/nps.h).
//
// A subset run is nps_score_cohort_def on the cohort that holds only the kept samples' columns: every row's decisions
// (nimpress.nim:565, :471) and its cohort-frequency imputation value come from tallyAlleles (:32-47) over the KEPT samples.
// Both formats that take it already have a "tallies first, then decide, then accumulate" route, whose decision kernels take
// the sample count as a number and whose accumulation kernels never ask where the tallies came from.  So all that is new is
// the two tally kernels counted under a sample mask -- the strip layout's here, the dosage rows' beside the kernel it mirrors
// (ds_tally_masked_kernel, nps_ds.hip, launched by launch_ds_tally) -- and the gather of the kept samples' scores.  The accumulation
// runs over every sample of the cohort as it always does; what it leaves at the dropped samples' positions is never read.
//
// The mask (nps_subset_mask.h) is wave-uniform wherever it is loaded: a unit of the strip layout (32 samples x 128 rows) has
// ONE 64-bit word, and a dropped sample reads as code 0 -- like the padding samples of the layout's last unit.
#include <algorithm>

#include "nps_kernels.h"
#include "nps_mx_common.h"

namespace nps {

// ---- NPS_FMT_GT2X: mx_tally_kernel (nps_mx.hip) under a mask ----------------------------------------------------------
// Same grid, same geometry: one workgroup = one superblock x a group of 16 strips, a lane holds rows 2 lane, 2 lane + 1 of
// every unit its wave reads, the four waves meet in LDS, one word (nmissing << 28 | neffect) per row and workgroup.  Four
// units per wave in flight; a unit none of whose samples is kept is not read.
__global__ __launch_bounds__(256) void mx_tally_masked_kernel(const v4u *__restrict__ units, uint64_t n_sb_cohort, uint32_t sb0,
                                                              uint32_t P, uint32_t nu_last,
                                                              const unsigned long long *__restrict__ unit_mask,
                                                              unsigned long long *__restrict__ tally) {
    __shared__ uint32_t s_eff[128], s_mis[128];
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t sb = blockIdx.x, grp = blockIdx.y;
    if (tid < 128) s_eff[tid] = s_mis[tid] = 0u;
    __syncthreads();
    MxTal t;
    const uint32_t s_end = min(P, grp * 16 + 16);
    for (uint32_t strip = grp * 16; strip < s_end; ++strip) {
        const uint32_t nu = strip == P - 1 ? nu_last : 64u;
        const v4u *base = units + ((uint64_t)strip * 64 * n_sb_cohort + (uint64_t)(sb0 + sb) * nu) * 64 + lane;
        const unsigned long long *mask = unit_mask + (uint64_t)strip * 64;  // (strip * 64 + u < units of the cohort for u < nu)
        for (uint32_t u0 = wave; u0 < nu; u0 += 16) {
            unsigned long long mk[4];
            v4u w[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) mk[j] = u0 + 4 * j < nu ? mask[u0 + 4 * j] : 0ull;  // (four scalar loads, one wait)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                w[j] = v4u{0u, 0u, 0u, 0u};
                if (mk[j]) w[j] = __builtin_nontemporal_load(base + (uint64_t)(u0 + 4 * j) * 64);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t ml = (uint32_t)mk[j], mh = (uint32_t)(mk[j] >> 32);
                mx_tally_unit(t, v4u{w[j].x & ml, w[j].y & mh, w[j].z & ml, w[j].w & mh});
            }
        }
    }
    mx_tally_commit(t, s_eff, s_mis, tally + (uint64_t)sb * 128);
}

hipError_t launch_mx_tally_masked(hipStream_t st, const MxPlan &plan, const void *d_units, uint64_t n_sb_cohort, uint64_t sb0,
                                  const unsigned long long *d_unit_mask, unsigned long long *d_tally) {
    if (!plan.ok || !d_unit_mask) return hipErrorInvalidValue;
    (void)hipGetLastError();
    const uint32_t groups = (plan.P + 15) / 16;
    for (uint32_t s = 0; s < plan.n_sb; s += 1u << 30) {  // (grid.x holds 2^31 - 1 blocks)
        const uint32_t k = std::min<uint32_t>(1u << 30, plan.n_sb - s);
        hipLaunchKernelGGL(mx_tally_masked_kernel, dim3(k, groups), dim3(256), 0, st, (const v4u *)d_units, n_sb_cohort,
                           (uint32_t)sb0 + s, plan.P, plan.nu_last, d_unit_mask, d_tally + (uint64_t)s * 128);
    }
    return hipGetLastError();
}

// ---- the kept samples' scores, in cohort order ------------------------------------------------------------------------
// scores: the n values finish_kernel made (nimpress.nim:643-649); kept sample i goes to prefix[i / 32] + the kept samples
// in front of it inside its word (nps_subset_mask.h: subset_position), a position below n_kept
__global__ __launch_bounds__(256) void subset_gather_kernel(const double *__restrict__ scores, uint64_t n,
                                                            const uint32_t *__restrict__ bits,
                                                            const uint32_t *__restrict__ prefix, double *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t w = bits[i >> 5], b = (uint32_t)i & 31u;
    if (!((w >> b) & 1u)) return;
    out[(uint64_t)prefix[i >> 5] + (uint32_t)__popc(w & ((1u << b) - 1u))] = scores[i];
}

hipError_t launch_subset_gather(hipStream_t st, const double *d_scores, uint64_t n, const uint32_t *d_bits,
                                const uint32_t *d_prefix, double *d_out) {
    if (n == 0) return hipSuccess;
    if (!d_bits || !d_prefix) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(subset_gather_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, d_scores, n, d_bits, d_prefix,
                       d_out);
    return hipGetLastError();
}

}  // namespace nps
