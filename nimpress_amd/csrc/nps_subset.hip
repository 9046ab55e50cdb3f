// nps_subset.hip -- scoring a chosen subset of a resident cohort's samples (nps_score_cohort_def_subset, include/nps.h).
//
// A subset run is nps_score_cohort_def on the cohort that holds only the kept samples' columns: every row's decisions
// (nimpress.nim:565, :471) and its cohort-frequency imputation value come from tallyAlleles (:32-47) over the KEPT samples.
// Both formats that take it already have a "tallies first, then decide, then accumulate" route, whose decision kernels take
// the sample count as a number and whose accumulation kernels never ask where the tallies came from.  So all that is new is
// here: the two tally kernels counted under a sample mask, and the gather of the kept samples' scores.  The accumulation
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
    uint32_t xa = 0, ya = 0, za = 0, xb = 0, yb = 0, zb = 0;
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
                const uint32_t wx = w[j].x & ml, wy = w[j].y & mh, wz = w[j].z & ml, ww = w[j].w & mh;
                const uint32_t sx = wx >> 1, sy = wy >> 1, sz = wz >> 1, sw = ww >> 1;
                xa = bcnt_acc(wy, bcnt_acc(wx, xa));
                ya = bcnt_acc((wx & 0xAAAAAAAAu) | (sy & 0x55555555u), ya);
                za = bcnt_acc((wx & sx & 0x55555555u) | ((wy & sy & 0x55555555u) << 1), za);
                xb = bcnt_acc(ww, bcnt_acc(wz, xb));
                yb = bcnt_acc((wz & 0xAAAAAAAAu) | (sw & 0x55555555u), yb);
                zb = bcnt_acc((wz & sz & 0x55555555u) | ((ww & sw & 0x55555555u) << 1), zb);
            }
        }
    }
    atomicAdd(&s_eff[2 * lane], xa + ya - 3u * za);
    atomicAdd(&s_mis[2 * lane], za);
    atomicAdd(&s_eff[2 * lane + 1], xb + yb - 3u * zb);
    atomicAdd(&s_mis[2 * lane + 1], zb);
    __syncthreads();
    if (tid < 128)
        atomicAdd(&tally[(uint64_t)sb * 128 + tid], ((unsigned long long)s_mis[tid] << 28) | (unsigned long long)s_eff[tid]);
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

// ---- NPS_FMT_DS32: ds_tally_kernel (nps_ds.hip) under a mask ----------------------------------------------------------
// One 256-thread block per row.  A dropped sample adds neither to nmiss nor to the sum; a thread adds its kept terms in the
// order ds_tally_kernel adds them, and the wave and block combine is that kernel's: with every sample kept the sum has the
// same bits.  bits: one bit per sample (nps_subset_mask.h); the four samples of a 16-byte load share a nibble.
static __device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
static __device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void ds_tally_masked_kernel(const float *__restrict__ ds, uint64_t stride_f, uint64_t n,
                                                              const nps_row_desc *__restrict__ desc, uint64_t n_rows,
                                                              const uint32_t *__restrict__ bits, DsTally *__restrict__ out) {
    __shared__ double s_sum[4];
    __shared__ uint32_t s_cnt[4];
    const uint64_t row = blockIdx.x;
    if (row >= n_rows) return;
    const bool rie = desc[row].ref_is_effect == 1;  // bit 1 set: the row already counts the effect allele
    const float4 *p = reinterpret_cast<const float4 *>(ds + row * stride_f);
    const uint64_t n4 = (n + 3) / 4;  // rows are zero padded to a multiple of 64 floats
    uint32_t cnt = 0;
    double sum = 0.0;
    auto nibble = [&](uint64_t v) { return (bits[v >> 3] >> (4 * (uint32_t)(v & 7))) & 15u; };  // (v < n4: word v / 8 < ceil(n / 32))
    auto take = [&](const float4 q, uint32_t nib, uint64_t v) {
        const float e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (v * 4 + k < n && ((nib >> k) & 1u)) {
                if (isnan(e[k]))
                    cnt += 1;
                else
                    sum += rie ? 2.0 - (double)e[k] : (double)e[k];
            }
        }
    };
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    // 8 independent 16-byte loads in flight per thread (the per-thread sum order stays v-ascending); the 1 KiB a wave
    // loads at a time is not read when none of its 256 samples is kept (a wave-uniform decision)
    uint64_t v = threadIdx.x;
    for (; v + 7 * 256 < n4; v += 8 * 256) {
        float4 q[8];
        uint32_t nib[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) nib[u] = nibble(v + u * 256);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            q[u] = zero;
            if (__any(nib[u] != 0u)) q[u] = p[v + u * 256];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) take(q[u], nib[u], v + u * 256);
    }
    for (; v < n4; v += 256) {
        const uint32_t nib = nibble(v);
        take(p[v], nib, v);
    }
    sum = wave_sum_f64(sum);
    cnt = wave_sum_u32(cnt);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_sum[w] = sum;
        s_cnt[w] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        DsTally t;
        t.nmiss = (unsigned long long)s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        t.neff = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
        out[row] = t;
    }
}

hipError_t launch_ds_tally_masked(hipStream_t st, const float *d_ds, uint64_t stride_f, uint64_t n, const nps_row_desc *d_desc,
                                  uint64_t n_rows, const uint32_t *d_bits, DsTally *d_tally) {
    if (n_rows == 0) return hipSuccess;
    if (n_rows > 0x7fffffffull || !d_bits) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(ds_tally_masked_kernel, dim3((uint32_t)n_rows), dim3(256), 0, st, d_ds, stride_f, n, d_desc, n_rows, d_bits,
                       d_tally);
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
