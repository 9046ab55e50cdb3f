// nps_mx_route.h -- the host-side policy of the strip layout NPS_FMT_GT2X, free of HIP (plain C++: tests/native/route_driver.cpp
// compiles it with g++): the layout's geometry, the plan of a run (strips, row teams, the grid its kernel runs on) and the
// ROUTE nps_score_cohort_def takes -- which kernel scores the run and where its row tallies come from.  Internal header.
#pragma once
#include <algorithm>
#include <cstdint>

namespace nps {

// cohort = [strip of 2048 samples][superblock of 128 rows][unit of 32 samples][row][8 bytes]; codes 0, 1, 2 =
// dosage, 3 = missing; sample s of a unit in bits 2s, 2s+1 of the row's 8 bytes.  Every strip but the last has
// 64 units; the last has what is left.
struct MxGeom {
    uint64_t n_units = 0, n_sb = 0;
    uint32_t P = 0, nu_last = 0;
};
static inline MxGeom mx_geom(uint64_t n_samples, uint64_t n_rows) {
    MxGeom g;
    g.n_units = (n_samples + 31) / 32;
    g.n_sb = (n_rows + 127) / 128;
    g.P = (uint32_t)((g.n_units + 63) / 64);
    g.nu_last = g.P ? (uint32_t)(g.n_units - 64ull * (g.P - 1)) : 0u;
    return g;
}
constexpr uint32_t kFlushSb = 1024;  // superblocks between flushes of the float32 digit sums (131 072 rows x 75 < 2^24)

struct MxPlan {
    bool ok = false;
    bool given = false;  // the shape does not fit one cooperative grid (more strips than compute units): the row
                         // tallies come from launch_mx_tally, the accumulation runs as an ordinary grid (two reads)
    uint32_t P = 0, Q = 0, nu_last = 0, n_sb = 0, n_flush = 0;  // strips, row teams per strip (superblock k belongs to team k % Q)
    uint64_t cpart_floats = 0;  // digit sums handed to mx_fold_kernel
    // The strips the kernel of THIS plan runs on, resolved here once: the launcher, the fold of the digit sums and
    // nps_fused_geometry read them (P / nu_last above address the layout).  The single-read kernel may cut the unit sequence
    // into strips of grid_U = 62 units instead of the layout's 64 where that puts more compute units to work (500 000
    // samples: 253 strips instead of 245): grid_P strips, the last of grid_nu_last units.  Every other kernel: the layout's.
    uint32_t grid_P = 0, grid_nu_last = 0, grid_U = 64;
};

// two_pass: plan the tally + accumulate pair whatever the shape (NPS_MODE_TWOPASS, tallies given); cus: compute units
// force_q: that many row teams for the given-tallies grid (diagnostics builds; 0: the choice below)
static inline MxPlan mx_plan_for(int cus, uint64_t n_samples, uint64_t n_rows, bool two_pass, uint64_t force_q = 0) {
    MxPlan plan;
    if (cus <= 0 || n_samples == 0 || n_rows == 0 || n_samples >= (1ull << 27)) return plan;
    const MxGeom gm = mx_geom(n_samples, n_rows);
    if (gm.n_sb > 0x1fffffffull || gm.P > 65535u) return plan;
    plan.P = gm.P;
    plan.nu_last = gm.nu_last;
    plan.n_sb = (uint32_t)gm.n_sb;
    // One strip per compute unit, the whole grid resident (8-bit arrival count): the single-read kernel.  Fewer strips
    // than compute units: Q row teams per strip fill the chip (superblock k belongs to team k % Q).  More strips than
    // compute units (N > 2048 x CUs): the tallies come from their own pass and the accumulation runs as an ordinary
    // grid of P x Q independent workgroups, about four per compute unit for an even tail.
    plan.given = two_pass || gm.P > (uint32_t)cus || gm.P > 255;
    uint64_t q = (uint64_t)cus / gm.P;
    if (plan.given) {
        // independent workgroups, one resident per compute unit at a time: P x Q of them run in ceil(P Q / CUs) rounds.
        // Of the team counts that give between two and eight rounds, the one whose last round is fullest (147 strips:
        // Q = 7 would be 1029 workgroups = four rounds and five stragglers; Q = 12 is 1764 = seven rounds, 98 % full)
        const uint64_t lo = std::max<uint64_t>(1, ((uint64_t)2 * cus + gm.P - 1) / gm.P), hi = std::max<uint64_t>(lo, (uint64_t)8 * cus / gm.P);
        double best = -1.0;
        q = lo;
        for (uint64_t t = lo; t <= hi; ++t) {
            const uint64_t wg = (uint64_t)gm.P * t, rounds = (wg + cus - 1) / cus;
            const double fill = (double)wg / (double)(rounds * cus);
            if (fill > best + 1e-9) {
                best = fill;
                q = t;
            }
        }
        if (force_q) q = force_q;
    }
    q = std::max<uint64_t>(1, std::min<uint64_t>(q, gm.n_sb));
    plan.Q = (uint32_t)q;
    const uint64_t n_t = (gm.n_sb + q - 1) / q;  // superblocks of the longest team
    plan.n_flush = (uint32_t)((n_t + kFlushSb - 1) / kFlushSb);
    // virtual strips of 62 units for the first form: only where one row team per strip is all there is (more than half the
    // compute units are strips already) and the finer cut still fits the resident grid
    plan.grid_U = 64;
    plan.grid_P = gm.P;
    plan.grid_nu_last = gm.nu_last;
    if (!plan.given && q == 1) {
        const uint64_t total_units = (uint64_t)(gm.P - 1) * 64 + gm.nu_last, pv = (total_units + 61) / 62;
        if (pv > gm.P && pv <= (uint64_t)cus && pv <= 255) {
            plan.grid_U = 62;
            plan.grid_P = (uint32_t)pv;
            plan.grid_nu_last = (uint32_t)(total_units - (pv - 1) * 62);
        }
    }
    plan.cpart_floats = (uint64_t)plan.n_flush * q * plan.grid_P * 64 * 2 * 256;
    plan.ok = true;
    return plan;
}

// ---- the route of a NPS_FMT_GT2X run --------------------------------------------------------------------------------
// Two kernels score a run: the single-read kernel that counts the rows' tallies IN the PASS (a cooperative grid, plan
// without `given`), and the accumulation with the tallies GIVEN (an ordinary grid, plan with `given`).
enum class MxRoute {
    InPass,        // single-read kernel
    InPassKeep,    // single-read kernel, and its epilogue keeps the run's tallies with the cohort (published after the pass)
    GivenKept,     // given-tallies kernel on the tallies kept with the cohort: one read
    GivenTallied,  // a tally pass over the run's rows, then the given-tallies kernel: two reads
};
constexpr int kMxModeAuto = 0, kMxModeTwoPass = 1, kMxModeFused = 2;  // NPS_MODE_* (nps_kernels.h holds them together)
struct MxRouteIn {
    int mode = kMxModeAuto, cus = 0;  // cus: compute units of the device
    uint64_t n_samples = 0, m = 0, n_rows_cohort = 0, cohort_row0 = 0;  // the run: m rows from cohort_row0
    bool run_tallies_valid = false;  // every superblock of the run carries its tallies
    bool tallies_asked = false;      // nps_cohort_keep_tallies, or a pass that kept them
    uint32_t expect_passes = 0;      // nps_cohort_expect_passes
};
struct MxRouted {
    bool ok = false;             // false: the shape is beyond the strip kernels
    bool refused_fused = false;  // NPS_MODE_FUSED on a shape without a resident grid
    MxRoute route = MxRoute::InPass;
    bool count_cohort_first = false;  // GivenKept: count the cohort's missing tallies (once, under its mutex) before the run
    MxPlan plan;                      // what the route's kernel runs with (planned two_pass for the Given* routes)
};
static inline MxRouted mx_route(const MxRouteIn &in) {
    MxRouted r;
    const MxPlan p1 = mx_plan_for(in.cus, in.n_samples, in.m, false);  // the in-pass plan
    if (!p1.ok) return r;
    r.ok = true;
    // (only where a strip has ONE row team -- more than 128 strips, 262 144 samples: with several teams per strip the
    //  given-tallies kernel is no faster than the pass that counts them -- 250 000 samples 11.3 against 11.4 ms,
    //  200 000 equal -- and slower below: 100 000 samples 5.05 against 4.27 ms, profiles/r06_harvest.txt)
    const bool one_team = p1.given || p1.Q == 1;
    if (in.mode == kMxModeTwoPass) {
        r.route = MxRoute::GivenTallied;  // (never the kept tallies: the mode asks for both reads)
    } else if (in.mode == kMxModeFused) {
        // more strips than compute units: the single-read kernel cannot hold the grid resident
        r.refused_fused = p1.given;
    } else if (in.run_tallies_valid) {
        // A run whose superblocks all carry their tallies is scored with them given -- the "two-pass" plan (independent
        // workgroups) without its tally pass -- when the tallies were asked for (nps_cohort_keep_tallies, a pass that kept
        // them: any size), or when they came with the rows (upload, upload_bed, convert) and a strip has ONE row team:
        // only there is the given-tallies kernel faster than the pass that counts them.  Smaller cohorts keep and serve
        // their write-time tallies (nps_cohort_row_tallies) and are scored in the pass.
        if (in.tallies_asked || one_team) r.route = MxRoute::GivenKept;
    } else {
        // Does the single-read kernel's resident grid cover the chip at this size, and will the cohort be scored again?
        //   * a resident grid exists (P <= compute units) and the run covers the whole cohort: the pass counts the tallies
        //     anyway -- where later passes want them given (the grid covers less than nine tenths of the chip, or the
        //     caller said nps_cohort_expect_passes >= 2) its epilogue KEEPS them with the cohort (InPassKeep): the first
        //     run is one read, every later one runs with the tallies given (round 6; until then the first run of such
        //     a size was a tally pass + a given-tallies pass: two reads);
        //   * no resident grid (more strips than compute units), or a partial run of at least a quarter of the cohort:
        //     count the cohort's tallies once (one more read) and keep them (the cohort's own cache: rewriting rows
        //     drops it); shorter runs tally just their own rows (two reads of those rows).
        // (nine tenths, by measurement: at 400 000 samples -- 196 strips, 77 % of the chip -- the in-pass kernel runs at
        //  0.64-0.67 of the roofline and the same cohort with its tallies given at 0.73-0.75; until round 6, when keeping
        //  the tallies still cost a pass of its own, the line was drawn at seven tenths)
        const bool covers = !p1.given && (uint64_t)p1.P * p1.Q * 10 >= (uint64_t)in.cus * 9;
        const bool want_kept = one_team && (!covers || in.expect_passes >= 2);
        const bool whole = in.cohort_row0 == 0 && in.m == in.n_rows_cohort;
        if (want_kept && !p1.given && whole && in.m >= 1024) {
            r.route = MxRoute::InPassKeep;
        } else if (want_kept && (p1.given || (!covers && in.m >= 16384)) && in.m * 4 >= in.n_rows_cohort) {
            r.route = MxRoute::GivenKept;
            r.count_cohort_first = true;
        } else if (p1.given) {
            r.route = MxRoute::GivenTallied;  // AUTO takes the tally + accumulate pair (two reads)
        }
    }
    const bool two_pass = r.route == MxRoute::GivenKept || r.route == MxRoute::GivenTallied;
    r.plan = two_pass ? mx_plan_for(in.cus, in.n_samples, in.m, true) : p1;
    return r;
}

}  // namespace nps
