// subset_driver.cpp -- prints the sample mask (nimpress_amd/csrc/nps_subset_mask.h) the library makes from keep bytes, for
// tests/test_subset_mask.py.  Plain C++ (g++ -fsanitize=address,undefined): the header needs neither HIP nor a device.
//
// stdin, one query per line:   <n_samples> <keep bytes as 2 n_samples hexadecimal digits>
// stdout, one line per query:  n_kept | the 1-bit words | the unit words | the prefix words | the position of every kept sample
// (hexadecimal words; the four lists separated by " | ")
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "nps_subset_mask.h"

static int hexval(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

int main() {
    unsigned long long n;
    std::string hex;
    while (std::cin >> n >> hex) {
        if (hex.size() != 2 * n) {
            std::fprintf(stderr, "query of %llu samples carries %zu digits\n", n, hex.size());
            return 2;
        }
        // exactly n bytes on the heap: the sanitizer sees a read beyond the caller's buffer
        std::vector<uint8_t> keep(n);
        for (unsigned long long i = 0; i < n; ++i) {
            const int h = hexval(hex[2 * i]), l = hexval(hex[2 * i + 1]);
            if (h < 0 || l < 0) return 2;
            keep[i] = (uint8_t)(h * 16 + l);
        }
        const nps::SubsetMask m = nps::subset_mask(keep.data(), n);
        std::printf("%llu |", (unsigned long long)m.n_kept);
        for (uint32_t w : m.bits) std::printf(" %x", w);
        std::printf(" |");
        for (uint64_t w : m.unit) std::printf(" %llx", (unsigned long long)w);
        std::printf(" |");
        for (uint32_t w : m.prefix) std::printf(" %x", w);
        std::printf(" |");
        for (unsigned long long i = 0; i < n; ++i)
            if (keep[i]) std::printf(" %llu", (unsigned long long)nps::subset_position(m, i));
        std::printf("\n");
    }
    return 0;
}
