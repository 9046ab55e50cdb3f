// nps_pl.hip -- FORMAT/PL (phred-scaled genotype likelihoods) of a diploid record -> the float32 row of the effect
// allele's expected count, on the device (build-defined extension: the reference decodes GT only; the arithmetic is
// stated in include/nps.h above nps_push_pl).  The row "already counts the effect allele" (NPS_RIE_COUNTS_EFFECT) and is
// scored by the DS kernels, like the rows of decode_gt_to_ds_kernel.
//
// The source is a staging slot in pinned host memory, read over PCIe.  A sample's G = A (A + 1) / 2 values are
// G x sizeof(T) bytes -- 3 for the common int8 biallelic record -- so a load per thread would be narrow and unaligned.
// A workgroup of 256 threads therefore takes the contiguous 256 x G x sizeof(T) bytes of its 256 samples with 16-byte
// loads into LDS (the chunk starts at a multiple of 256 bytes; the last chunk's tail is read rounded up to 16 bytes,
// which the slot is sized for), keeps the 256 likelihoods (2 KB) beside them, and every thread decodes its own sample
// from LDS.  No array is indexed per thread: the kernel uses no scratch memory (tests/test_pl_isa.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>

#include "nps_kernels.h"

namespace nps {

// T[k] = 10^(-k/10), k = 0 .. 255: built once on the host (the values nps_pl_likelihoods hands out), one copy per device
static __device__ double g_pl_table[256];

const double *pl_likelihood_table() {
    static double table[256];
    static std::once_flag once;
    std::call_once(once, [] {
        for (int k = 0; k < 256; ++k) table[k] = pow(10.0, -(double)k / 10.0);
    });
    return table;
}

template <typename T>
__global__ __launch_bounds__(256) void decode_pl_kernel(const T *__restrict__ src, uint64_t n, int n_alleles, int eaidx,
                                                        float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pl_lds[];
    double *const lik = reinterpret_cast<double *>(pl_lds);  // [256]
    unsigned char *const raw = pl_lds + 256 * sizeof(double);
    const uint32_t tid = threadIdx.x;
    const uint32_t G = (uint32_t)(n_alleles * (n_alleles + 1) / 2);
    const uint32_t sample_bytes = G * (uint32_t)sizeof(T);
    const uint64_t s0 = (uint64_t)blockIdx.x * 256;
    const uint64_t left = n - s0;  // (the grid has no block beyond the last sample)
    const uint32_t here = left < 256 ? (uint32_t)left : 256u;
    const uint32_t vecs = (here * sample_bytes + 15u) / 16u;  // <= 16 x sample_bytes: inside the LDS chunk
    const uint4 *const g = reinterpret_cast<const uint4 *>(reinterpret_cast<const unsigned char *>(src) + s0 * sample_bytes);
    uint4 *const l = reinterpret_cast<uint4 *>(raw);
    lik[tid] = g_pl_table[tid];
    for (uint32_t i = tid; i < vecs; i += 256) l[i] = g[i];
    __syncthreads();
    if (tid >= here) return;
    const T *const p = reinterpret_cast<const T *>(raw + tid * sample_bytes);
    double num = 0.0, den = 0.0;
    int32_t lo = 0x7fffffff, hi = (int32_t)0x80000000;
    uint32_t j = 0, k = 0;  // genotype g = (j, k), j <= k, in the order of the VCF specification: g = k (k + 1) / 2 + j
    for (uint32_t gi = 0; gi < G; ++gi) {
        const int32_t v = (int32_t)p[gi];
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
        const double w = lik[v < 0 ? 0 : (v > 255 ? 255 : v)];
        const int cnt = (int)(j == (uint32_t)eaidx) + (int)(k == (uint32_t)eaidx);
        num = num + (double)cnt * w;
        den = den + w;
        if (j == k) {
            j = 0;
            ++k;
        } else {
            ++j;
        }
    }
    // missing: a missing / end-of-vector value (negative in every width), or a flat vector
    out[s0 + tid] = (lo < 0 || lo == hi) ? __int_as_float(0x7fc00000) : (float)(num / den);
}

hipError_t launch_decode_pl(hipStream_t st, const void *src, int elem_bytes, uint64_t n, int n_alleles, int eaidx,
                            float *d_out) {
    if (n == 0) return hipSuccess;
    if (n_alleles < 2 || n_alleles > 8 || eaidx < 0 || eaidx >= n_alleles) return hipErrorInvalidValue;
    // the table of this device, uploaded before its first launch (a blocking copy: complete when it returns)
    static std::mutex mu;
    static bool uploaded[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    {
        std::lock_guard<std::mutex> lk(mu);
        if (!uploaded[dev]) {
            e = hipMemcpyToSymbol(HIP_SYMBOL(g_pl_table), pl_likelihood_table(), 256 * sizeof(double));
            if (e != hipSuccess) return e;
            uploaded[dev] = true;
        }
    }
    (void)hipGetLastError();
    const dim3 grid((uint32_t)((n + 255) / 256)), block(256);
    const size_t lds = 256 * sizeof(double) + (size_t)256 * (size_t)(n_alleles * (n_alleles + 1) / 2) * (size_t)elem_bytes;
    switch (elem_bytes) {
    case 1:
        hipLaunchKernelGGL(decode_pl_kernel<int8_t>, grid, block, lds, st, (const int8_t *)src, n, n_alleles, eaidx, d_out);
        break;
    case 2:
        hipLaunchKernelGGL(decode_pl_kernel<int16_t>, grid, block, lds, st, (const int16_t *)src, n, n_alleles, eaidx, d_out);
        break;
    case 4:
        hipLaunchKernelGGL(decode_pl_kernel<int32_t>, grid, block, lds, st, (const int32_t *)src, n, n_alleles, eaidx, d_out);
        break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace nps
