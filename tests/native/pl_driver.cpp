// Test driver for the FORMAT/PL readers (no GPU, no libnps call: links the reader units of
// nimpress_amd/build.py's HOST_READER_SOURCES only).
//   pl_driver <file> [<file> ...]
// opens every genotype file under NIMPRESS_FORMAT=PL (set here) and prints, per file, either
//   refused <file>: <the reader's message>
// or one line per record
//   rec <contig>:<pos> src=PL|GT|DS per=<values per sample> bytes=<element bytes> pl=<v,v,..;v,v,..;..>
// with every PL value widened to int32 (missing 0x80000000 -> "M", end of vector -> "E").  The status is 0 whatever the
// files hold: a file the readers refuse is a message, never a crash.  Built with -fsanitize=address,undefined by
// tests/test_host_pl.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

#include "../../nimpress_amd/csrc/host/nimpress_host.hpp"

using namespace nimpress;

static long long plValue(const Variant &v, size_t i) {
    switch (v.pl_bytes) {
    case 1: {
        int8_t x;
        memcpy(&x, &v.pl_raw[i], 1);
        return x == INT8_MIN ? INT32_MIN : (x == INT8_MIN + 1 ? INT32_MIN + 1 : x);
    }
    case 2: {
        int16_t x;
        memcpy(&x, &v.pl_raw[2 * i], 2);
        return x == INT16_MIN ? INT32_MIN : (x == INT16_MIN + 1 ? INT32_MIN + 1 : x);
    }
    default: {
        int32_t x;
        memcpy(&x, &v.pl_raw[4 * i], 4);
        return x;
    }
    }
}

int main(int argc, char **argv) {
    setenv("NIMPRESS_FORMAT", "PL", 1);
    for (int a = 1; a < argc; ++a) {
        try {
            VCF vcf;
            if (!vcf.open(argv[a])) {
                printf("refused %s: cannot open\n", argv[a]);
                continue;
            }
            const size_t ns = vcf.samples.size();
            for (const Variant &v : vcf.records) {
                printf("rec %s:%lld src=%s per=%d bytes=%d pl=", v.contig.c_str(), (long long)v.pos,
                       v.has_pl ? "PL" : (v.has_ds ? "DS" : "GT"), v.pl_per_sample, v.has_pl ? v.pl_bytes : 0);
                if (v.has_pl) {
                    if (v.pl_raw.size() != ns * (size_t)v.pl_per_sample * (size_t)v.pl_bytes) {
                        printf("BAD SIZE\n");
                        return 1;
                    }
                    for (size_t i = 0; i < ns; ++i) {
                        for (int k = 0; k < v.pl_per_sample; ++k) {
                            const long long x = plValue(v, i * (size_t)v.pl_per_sample + (size_t)k);
                            if (k) printf(",");
                            if (x == INT32_MIN)
                                printf("M");
                            else if (x == INT32_MIN + 1)
                                printf("E");
                            else
                                printf("%lld", x);
                        }
                        if (i + 1 < ns) printf(";");
                    }
                }
                printf("\n");
            }
        } catch (const std::exception &e) {
            printf("refused %s: %s\n", argv[a], e.what());
        }
    }
    return 0;
}
