// nps_ds_common.h -- device code the dosage sources share (nps_ds.hip, nps_multi_ds.hip): the element decode of the two
// dosage formats, the row tally kernel with its summation tree, the per-row record of the accumulation kernels.  Internal header.
#pragma once
#include <type_traits>

#include "nps_kernels.h"

namespace nps {

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

// four neighbouring samples of a row as they lie in memory, and the float32 dosage an element stands for
template <typename E>
struct DsElem;
template <>
struct DsElem<float> {
    typedef float v4 __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ float value(float e) { return e; }
};
template <>
struct DsElem<uint16_t> {  // NPS_FMT_DS16: k = dosage x 10^4, 0xFFFF = missing (ds16_value: nps_kernels.h)
    typedef unsigned short v4 __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ float value(unsigned short k) {
        return k == 0xffffu ? __int_as_float(0x7fc00000) : ds16_value(k);
    }
};

// THE SUMMATION TREE of a dosage row's tally: the unmasked dosage tallies are instantiations of this kernel, one
// 256-thread block per row, and nps_flush, the two-pass run, the subset run and nps_multi_row_tallies promise each other
// equal bits through it (tests/ds_tally_tree.py restates it in numpy from this comment).
//   * a lane-of-four v holds samples 4 v .. 4 v + 3 (one 16-byte load of float32, 8 bytes of DS16); thread t takes the
//     lanes-of-four t, t + 256, t + 512, .. in ascending order, samples k = 0 .. 3 of each in order: a missing sample
//     (NaN) counts, any other adds its float32 value, converted to float64, to the thread's float64 sum -- 2.0 - value
//     for a flipped row.  Eight loads are in flight while eight lanes-of-four are left for the thread (which changes
//     no order);
//   * the wave sum: for o = 32, 16, .. 1 lane l adds what lane l + o holds (__shfl_down: lanes past the end add their
//     own value, which never reaches lane 0);
//   * the block sum of the four waves' lane-0 values: ((s0 + s1) + s2) + s3.
// BOTH = false: one sum into DsTally::neff, flipped when the row's ref_is_effect == 1 (bit 1 set: the row already
// counts the effect allele).  BOTH = true: the plain and the flipped sum side by side (desc is not read) -- tallies that
// belong to the row, not to a definition.
// Rows are zero padded to a multiple of 64 elements, so a row's last lane-of-four lies inside it.
// A kernel template and not a device function under thin kernels: inlined from a function, the compiler issues the
// first of the eight loads seventh (s_waitcnt vmcnt(1) in front of the first add, not vmcnt(7)), and the float32
// kernel measured 0.7 % slower.
// One copy of the tree remains: ds_tally_masked_kernel (nps_ds.hip), the subset run's tally, keeps its own text because
// its instantiation of this template measured outside the yardstick; tests/test_gpu_tally_tree_ds.py
// holds it to this tree bit for bit.
template <typename E, bool BOTH>
__global__ __launch_bounds__(256) void ds_tally_kernel(const E *__restrict__ ds, uint64_t stride_e, uint64_t n,
                                                       const nps_row_desc *__restrict__ desc, uint64_t n_rows,
                                                       typename std::conditional<BOTH, MultiDsTally, DsTally>::type *__restrict__ out) {
    typedef typename DsElem<E>::v4 V4;
    __shared__ double s_sum[BOTH ? 8 : 4];  // [4 .. 7]: the flipped sums
    __shared__ uint32_t s_cnt[4];
    const uint64_t row = blockIdx.x;
    if (row >= n_rows) return;
    const bool rie = !BOTH && desc[row].ref_is_effect == 1;
    const V4 *p = reinterpret_cast<const V4 *>(ds + row * stride_e);
    const uint64_t n4 = (n + 3) / 4;
    uint32_t cnt = 0;
    double sum = 0.0, flp = 0.0;
    auto take = [&](const V4 q, uint64_t v) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float e = DsElem<E>::value(q[k]);
            if (v * 4 + k < n) {
                if (isnan(e)) {
                    cnt += 1;
                } else if (BOTH) {
                    sum += (double)e;
                    flp += 2.0 - (double)e;
                } else {
                    sum += rie ? 2.0 - (double)e : (double)e;
                }
            }
        }
    };
    uint64_t v = threadIdx.x;
    for (; v + 7 * 256 < n4; v += 8 * 256) {
        V4 q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) q[u] = p[v + u * 256];
#pragma unroll
        for (int u = 0; u < 8; ++u) take(q[u], v + u * 256);
    }
    for (; v < n4; v += 256) take(p[v], v);
    sum = wave_sum_f64(sum);
    if (BOTH) flp = wave_sum_f64(flp);
    cnt = wave_sum_u32(cnt);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_sum[w] = sum;
        if (BOTH) s_sum[4 + w] = flp;
        s_cnt[w] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        typename std::conditional<BOTH, MultiDsTally, DsTally>::type t;
        t.nmiss = (unsigned long long)s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        const double s = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
        if constexpr (BOTH) {
            t.sum = s;
            t.sum_flipped = ((s_sum[4] + s_sum[5]) + s_sum[6]) + s_sum[7];
        } else {
            t.neff = s;
        }
        out[row] = t;
    }
}

// the record the dosage accumulation kernels read per row (and per score), from the row's decision
static __device__ __forceinline__ DsRowP ds_row_record(const RowDecision &d, double beta, bool flip) {
    DsRowP r;
    r.beta = beta;
    r.imp = d.mode == 1 ? d.imp : 0.0;
    r.cst = d.mode == 2 ? d.imp : 0.0;
    r.mode = d.mode;
    r.rie = flip ? 1 : 0;
    return r;
}

}  // namespace nps
