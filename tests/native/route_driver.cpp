// route_driver.cpp -- answers queries about the strip path's host policy (nimpress_amd/csrc/nps_mx_route.h) for
// tests/test_mx_route.py.  It includes that header and nothing else of the library: that it compiles with plain g++ is
// the proof that the policy needs neither HIP nor a device.  One query per line on stdin, one answer line each:
//   route <cus> <n_samples> <m> <n_rows_cohort> <row0> <valid> <asked> <expect_passes> <mode>
//       -> <ok> <refused_fused> <route> <count_cohort_first> <given> <P> <Q> <grid_P> <grid_nu_last> <grid_U>
//   plan <cus> <n_samples> <n_rows> <two_pass>
//       -> <ok> <given> <P> <Q> <grid_P> <grid_nu_last> <grid_U>
#include <cstdio>
#include <cstring>

#include "nps_mx_route.h"

static const char *route_name(nps::MxRoute r) {
    switch (r) {
    case nps::MxRoute::InPass: return "InPass";
    case nps::MxRoute::InPassKeep: return "InPassKeep";
    case nps::MxRoute::GivenKept: return "GivenKept";
    case nps::MxRoute::GivenTallied: return "GivenTallied";
    }
    return "?";
}

int main() {
    char what[16];
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "route")) {
            nps::MxRouteIn in;
            unsigned long long n, m, rows, row0;
            int valid, asked;
            unsigned expect;
            if (scanf("%d %llu %llu %llu %llu %d %d %u %d", &in.cus, &n, &m, &rows, &row0, &valid, &asked, &expect, &in.mode) != 9)
                return 2;
            in.n_samples = n;
            in.m = m;
            in.n_rows_cohort = rows;
            in.cohort_row0 = row0;
            in.run_tallies_valid = valid != 0;
            in.tallies_asked = asked != 0;
            in.expect_passes = expect;
            const nps::MxRouted r = nps::mx_route(in);
            printf("%d %d %s %d %d %u %u %u %u %u\n", (int)r.ok, (int)r.refused_fused, route_name(r.route),
                   (int)r.count_cohort_first, (int)r.plan.given, r.plan.P, r.plan.Q, r.plan.grid_P,
                   r.plan.grid_nu_last, r.plan.grid_U);
        } else if (!strcmp(what, "plan")) {
            int cus, two_pass;
            unsigned long long n, rows;
            if (scanf("%d %llu %llu %d", &cus, &n, &rows, &two_pass) != 4) return 2;
            const nps::MxPlan p = nps::mx_plan_for(cus, n, rows, two_pass != 0);
            printf("%d %d %u %u %u %u %u\n", (int)p.ok, (int)p.given, p.P, p.Q, p.grid_P, p.grid_nu_last, p.grid_U);
        } else {
            return 2;
        }
    }
    return 0;
}
