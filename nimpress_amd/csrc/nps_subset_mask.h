// nps_subset_mask.h -- a sample set (nps_sampleset, include/nps.h) as the device holds it, made from the caller's keep
// bytes.  Free of HIP (plain C++: tests/native/subset_driver.cpp compiles it with g++), like nps_mx_route.h.  Internal header.
//
//   bits    one bit per sample, sample i in bit i % 32 of word i / 32 (what the masked dosage tally and the gather read);
//           padded with zero words to a multiple of four words
//   unit    one 64-bit word per unit of the strip layout (32 samples, nps_mx_route.h): sample s of the unit in bits 2s, 2s + 1,
//           both set when the sample is kept -- the word a row of the unit (its 8 bytes of 2-bit codes) is ANDed with, so a
//           dropped sample reads as code 0 exactly like the padding samples of the last unit
//   prefix  the gather index: prefix[w] = kept samples in front of word w of `bits`; kept sample i goes to position
//           prefix[i / 32] + popcount(bits[i / 32] & ((1 << i % 32) - 1)) of the dense score vector (subset_position)
//
// Bits of samples beyond n_samples are zero in all three.
#pragma once
#include <cstdint>
#include <vector>

namespace nps {

struct SubsetMask {
    uint64_t n_samples = 0, n_kept = 0;
    std::vector<uint32_t> bits;
    std::vector<uint64_t> unit;
    std::vector<uint32_t> prefix;
};

// the 32 bits of a word of `bits`, each doubled: bit s -> bits 2s, 2s + 1
static inline uint64_t subset_spread2(uint32_t w) {
    uint64_t x = w;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x | (x << 1);
}

static inline uint32_t subset_popcount(uint32_t w) {
    w = w - ((w >> 1) & 0x55555555u);
    w = (w & 0x33333333u) + ((w >> 2) & 0x33333333u);
    return (((w + (w >> 4)) & 0x0F0F0F0Fu) * 0x01010101u) >> 24;
}

// keep: n_samples bytes, 0 = drop, anything else = keep
static inline SubsetMask subset_mask(const uint8_t *keep, uint64_t n_samples) {
    SubsetMask m;
    m.n_samples = n_samples;
    const uint64_t n_units = (n_samples + 31) / 32, n_words = (n_units + 3) / 4 * 4;
    m.bits.assign(n_words, 0u);
    m.unit.assign(n_units, 0ull);
    m.prefix.assign(n_words, 0u);
    for (uint64_t i = 0; i < n_samples; ++i)
        if (keep[i]) m.bits[i >> 5] |= 1u << (i & 31);
    uint64_t kept = 0;
    for (uint64_t w = 0; w < n_words; ++w) {
        m.prefix[w] = (uint32_t)kept;  // (n_samples < 2^31: nps_create)
        kept += subset_popcount(m.bits[w]);
        if (w < n_units) m.unit[w] = subset_spread2(m.bits[w]);
    }
    m.n_kept = kept;
    return m;
}

// where kept sample i goes in the dense vector (i < n_samples and kept)
static inline uint64_t subset_position(const SubsetMask &m, uint64_t i) {
    return (uint64_t)m.prefix[i >> 5] + subset_popcount(m.bits[i >> 5] & ((1u << (i & 31)) - 1u));
}

}  // namespace nps
