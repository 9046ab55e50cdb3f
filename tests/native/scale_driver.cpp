// scale_driver.cpp -- answers queries about the weight-scale rules (nimpress_amd/csrc/nps_scale.h) for
// tests/test_weight_scale.py.  It includes that header and nothing else of the library: that it compiles with plain g++ is
// the proof that the rules need neither HIP nor a device.  Doubles go in and out as the 16 hexadecimal digits of their bit
// pattern, so every comparison is exact.  One query per line on stdin, one answer line each:
//   span <eaf>                        -> <span>
//   special <beta> <eaf>              -> <0|1> <bound>
//   exp <bound>                       -> <F>
//   bands <m> {<beta> <eaf>} x m      -> <mx_bound> <k> {<special row>} x k {<band>} x m <u> {<band> <bound> <F>} x u
//   multi <S> <n_desc> <ND> {<kind> <beta> <eaf>} x S x n_desc
//                                     -> ok <no_scale> {<F>} x S
//                                      | refused <kind|beta|eaf|span> <score> <row> <minb> <maxb>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "nps_scale.h"

static bool read_double(double *d) {
    uint64_t bits;
    if (scanf("%" SCNx64, &bits) != 1) return false;
    memcpy(d, &bits, sizeof bits);
    return true;
}

static void print_double(double d) {
    uint64_t bits;
    memcpy(&bits, &d, sizeof bits);
    printf("%016" PRIx64, bits);
}

int main() {
    char what[16];
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "span")) {
            double eaf;
            if (!read_double(&eaf)) return 2;
            print_double(nps::imputation_span(eaf));
            printf("\n");
        } else if (!strcmp(what, "special")) {
            nps_row_desc r{};
            if (!read_double(&r.beta) || !read_double(&r.eaf)) return 2;
            double bound = -1.0;
            const bool sp = nps::mx_special(r, &bound);
            printf("%d ", (int)sp);
            print_double(bound);
            printf("\n");
        } else if (!strcmp(what, "exp")) {
            double bound;
            if (!read_double(&bound)) return 2;
            printf("%d\n", nps::mx_scale_exponent(bound));
        } else if (!strcmp(what, "bands")) {
            unsigned long long m;
            if (scanf("%llu", &m) != 1) return 2;
            std::vector<nps_row_desc> rows(m);
            for (auto &r : rows) {
                r = nps_row_desc{};
                r.kind = NPS_ROW_PRESENT;
                if (!read_double(&r.beta) || !read_double(&r.eaf)) return 2;
            }
            const nps::MxBandPlan p = nps::mx_band_plan(rows.data(), m);
            print_double(p.mx_bound);
            printf(" %zu", p.special.size());
            for (uint64_t j : p.special) printf(" %llu", (unsigned long long)j);
            for (int b : p.band) printf(" %d", b);
            printf(" %zu", p.used.size());
            for (size_t u = 0; u < p.used.size(); ++u) {
                printf(" %d ", p.used[u]);
                print_double(p.used_bound[u]);
                printf(" %d", nps::mx_scale_exponent(p.used_bound[u]));
            }
            printf("\n");
        } else if (!strcmp(what, "multi")) {
            int S, ND;
            unsigned long long n_desc;
            if (scanf("%d %llu %d", &S, &n_desc, &ND) != 3 || S < 1 || S > NPS_MULTI_MAX_SCORES) return 2;
            std::vector<nps_row_desc> rows((size_t)S * n_desc);
            for (auto &r : rows) {
                r = nps_row_desc{};
                if (scanf("%d", &r.kind) != 1 || !read_double(&r.beta) || !read_double(&r.eaf)) return 2;
            }
            const nps::MultiScale sc = nps::multi_scale(rows.data(), S, n_desc, ND);
            if (sc.refusal == nps::MultiScale::None) {
                printf("ok %d", sc.no_scale);
                for (int s = 0; s < S; ++s) printf(" %d", sc.F[s]);
                printf("\n");
            } else {
                static const char *const why[] = {"none", "kind", "beta", "eaf", "span"};
                printf("refused %s %d %llu ", why[sc.refusal], sc.score, (unsigned long long)sc.row);
                print_double(sc.minb);
                printf(" ");
                print_double(sc.maxb);
                printf("\n");
            }
        } else {
            return 2;
        }
    }
    return 0;
}
