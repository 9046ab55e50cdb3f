// decision_driver.cpp -- answers queries about the per-row decisions (nimpress_amd/csrc/nps_row_decision.h) for
// tests/test_row_decision.py.  It includes that header and nothing else of the library: that it compiles with plain g++
// is the proof that the rule every kernel calls needs neither HIP nor a device.  One query per line on stdin, one answer
// line each; a double travels as the 16 hexadecimal digits of its bit pattern (<..:x>), parameters as
// <prm> = <imp_locus> <imp_missing> <imp_sample> <maxmis:x> <mincs>:
//   nan                                            -> <row_nan():x>
//   thr <n> <rate:x>                               -> <maxmis_threshold>
//   over <k> <n> <rate:x>                          -> <over_maxmis>
//   row <prm> <spelling> <n> <nmiss> <neff:x> <eaf:x> <rie>
//       spelling 0: over = over_maxmis(nmiss, n, maxmis); 1: over = nmiss > maxmis_threshold(n, maxmis)
//       -> <used> <reason> <mode> <imp:x> | row_stat: <ngenotyped> <nmissing> <neffect:x> <used> <reason>
//   nodata <prm> <kind> <eaf:x> <rie>              -> <used> <reason> <mode> <imp:x>
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "nps_row_decision.h"

static double from_bits(uint64_t b) {
    double d;
    memcpy(&d, &b, sizeof d);
    return d;
}
static uint64_t bits(double d) {
    uint64_t b;
    memcpy(&b, &d, sizeof b);
    return b;
}
static bool read_params(nps::DevParams &p) {
    uint64_t rate;
    long long mincs;
    if (scanf("%" SCNd32 " %" SCNd32 " %" SCNd32 " %" SCNx64 " %lld", &p.imp_locus, &p.imp_missing, &p.imp_sample, &rate, &mincs) != 5)
        return false;
    p.max_missing_rate = from_bits(rate);
    p.min_cs = (double)mincs;  // as the engine converts nps_params.min_cs
    return true;
}

int main() {
    char what[16];
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "nan")) {
            printf("%016" PRIx64 "\n", bits(nps::row_nan()));
        } else if (!strcmp(what, "thr")) {
            uint64_t n, rate;
            if (scanf("%" SCNu64 " %" SCNx64, &n, &rate) != 2) return 2;
            printf("%" PRId64 "\n", nps::maxmis_threshold(n, from_bits(rate)));
        } else if (!strcmp(what, "over")) {
            uint64_t k, n, rate;
            if (scanf("%" SCNu64 " %" SCNu64 " %" SCNx64, &k, &n, &rate) != 3) return 2;
            printf("%d\n", (int)nps::over_maxmis(k, n, from_bits(rate)));
        } else if (!strcmp(what, "row")) {
            nps::DevParams p;
            int spelling, rie;
            uint64_t n, nmiss, neff, eaf;
            if (!read_params(p)) return 2;
            if (scanf("%d %" SCNu64 " %" SCNu64 " %" SCNx64 " %" SCNx64 " %d", &spelling, &n, &nmiss, &neff, &eaf, &rie) != 6) return 2;
            const bool over = spelling == 0 ? nps::over_maxmis(nmiss, n, p.max_missing_rate)
                                            : (int64_t)nmiss > nps::maxmis_threshold(n, p.max_missing_rate);
            const uint64_t ngen = n - nmiss;
            const nps::RowDecision d = nps::decide_row(p, over, from_bits(eaf), rie != 0, from_bits(neff), ngen);
            const nps_locus_stat s = nps::row_stat(d, ngen, nmiss, from_bits(neff));
            printf("%d %d %d %016" PRIx64 " %" PRIu64 " %" PRIu64 " %016" PRIx64 " %d %d\n", d.used, d.reason, d.mode, bits(d.imp),
                   s.ngenotyped, s.nmissing, bits(s.neffect), s.used, s.reason);
        } else if (!strcmp(what, "nodata")) {
            nps::DevParams p;
            int kind, rie;
            uint64_t eaf;
            if (!read_params(p)) return 2;
            if (scanf("%d %" SCNx64 " %d", &kind, &eaf, &rie) != 3) return 2;
            const nps::RowDecision d = nps::no_data_row(p, kind, from_bits(eaf), rie != 0);
            printf("%d %d %d %016" PRIx64 "\n", d.used, d.reason, d.mode, bits(d.imp));
        } else {
            return 2;
        }
    }
    return 0;
}
