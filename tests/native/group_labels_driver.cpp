// group_labels_driver.cpp -- prints what the library makes of the label bytes of a sample partition
// (nimpress_amd/csrc/nps_group_labels.h), for tests/test_group_labels.py.  Plain C++ (g++ -fsanitize=address,undefined): the
// header needs neither HIP nor a device.
//
// stdin, one query per line:   <n_samples> <n_groups> <label bytes as 2 n_samples hexadecimal digits>
// stdout, one line per query:  error sample group | the group sizes | the padded label bytes | the presence bytes
// (error: 0 good, 1 a bad label at `sample`, 2 every label 255, 3 `group` is empty; after an error the three lists are empty.
//  The bytes in hexadecimal; the lists separated by " | ")
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "nps_group_labels.h"

static int hexval(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

int main() {
    unsigned long long n;
    int n_groups;
    std::string hex;
    while (std::cin >> n >> n_groups >> hex) {
        if (hex.size() != 2 * n) {
            std::fprintf(stderr, "query of %llu samples carries %zu digits\n", n, hex.size());
            return 2;
        }
        // exactly n bytes on the heap: the sanitizer sees a read beyond the caller's buffer
        std::vector<uint8_t> label(n);
        for (unsigned long long i = 0; i < n; ++i) {
            const int h = hexval(hex[2 * i]), l = hexval(hex[2 * i + 1]);
            if (h < 0 || l < 0) return 2;
            label[i] = (uint8_t)(h * 16 + l);
        }
        const nps::GroupLabelCheck c = nps::group_labels_check(label.data(), n, n_groups);
        std::printf("%d %llu %d |", (int)c.error, (unsigned long long)c.sample, c.group);
        if (c.error != nps::kGroupLabelsOk) {
            std::printf(" | |\n");
            continue;
        }
        const nps::GroupLabels g = nps::group_labels(label.data(), n, n_groups);
        for (int k = 0; k < g.n_groups; ++k) std::printf(" %llu", (unsigned long long)g.size[k]);
        std::printf(" |");
        for (uint8_t b : g.label) std::printf(" %x", (unsigned)b);
        std::printf(" |");
        for (uint8_t b : g.present) std::printf(" %x", (unsigned)b);
        std::printf("\n");
    }
    return 0;
}
