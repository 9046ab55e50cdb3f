#!/usr/bin/env python3
"""dev tool: what does scoring every group of a sample partition in one pass (nps_score_cohort_def_groups) cost against the
entry points it replaces?  One synthetic NPS_FMT_DS32 cohort of --samples x --variants, then one NPS_FMT_DS16 cohort of the
same shape; for G = 1, 2, 5, 8 groups and random / contiguous labels the runs alternate, --reps of each, in one process on
one device: the grouped pass; the G subset runs (nps_score_cohort_def_subset with {label == k}, NPS_FMT_DS32 only -- the
NPS_FMT_DS16 rows are set against the float32 cohort's subset runs, there being no subset run of a DS16 cohort); one
whole-cohort run (NPS_MODE_TWOPASS on float32 rows, the single-read kernel on DS16 rows).  Times are HIP-event times of the
context's profile, best of --reps: the tally, the accumulation, and the whole pass (tally + params + accumulation + fused +
fold).  A small cohort is scored first with every kernel, so that no figure holds a first launch.
    python tools/qb_groups.py [--samples 200000] [--variants 100000] [--reps 3]"""
import argparse, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=200_000)
ap.add_argument("--variants", type=int, default=100_000)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
from nimpress_amd import capi
m, seed = a.variants, 20250301
rng = np.random.default_rng(seed)
SC = 4294967296.0
f = lambda x: np.minimum(np.floor(np.asarray(x, dtype=np.float64) * SC), 4294967295.0).astype(np.uint32)
eaf_c = np.round(rng.uniform(0.01, 0.5, m), 4)
th, tm, tmi = f(eaf_c * eaf_c + 2 * eaf_c * (1 - eaf_c)), f(eaf_c * eaf_c), f(rng.uniform(0, 0.08, m))
descs = capi.row_descs(np.round(rng.normal(0, 0.02, m), 4), np.round(rng.uniform(0.01, 0.9, m), 4), None,
                       (rng.uniform(size=m) < 0.3).astype(np.int32))
params = capi.make_params()
GS = (1, 2, 5, 8)


def make(fmt, nn, mm):
    co = capi.Cohort(nn, mm, fmt=fmt)
    for r0 in range(0, mm, 1 << 15):
        k = min(1 << 15, mm - r0)
        co.synth(r0, seed, th[r0:r0 + k], tm[r0:r0 + k], tmi[r0:r0 + k])
    return co


def labels(nn, G, kind):
    if kind == "random":
        return np.random.default_rng(G).integers(0, G, nn).astype(np.uint8)
    return (np.arange(nn, dtype=np.int64) * G // nn).astype(np.uint8)


def timed(sc, run):
    sc.reset()
    sc.profile_enable(True)
    sc.profile_get(reset=True)
    run()
    sc.sync()
    p = sc.profile_get(reset=True)
    return np.array([p.ms_tally, p.ms_accumulate, p.ms_tally + p.ms_params + p.ms_accumulate + p.ms_fused + p.ms_reduce])


def best(runs):
    return np.min(np.array(runs), axis=0)


def case(name, fmt, nn, mm, reps, subset_of=None, quiet=False):
    """subset_of: {(G, kind): whole-pass ms of the G subset runs} measured on the float32 cohort, for the DS16 rows"""
    co = make(fmt, nn, mm)
    sc, sd = capi.Scorer(nn, params), capi.ScoreDef(descs[:mm])
    whole_mode = capi.MODE_TWOPASS if fmt == capi.FMT_DS32 else capi.MODE_AUTO
    out = {}
    if not quiet:
        print("# %s %d x %d, best of %d, ms" % (name, nn, mm, reps), flush=True)
        print("# fmt  G labels     | grouped: tally accum whole | G subset runs: tally accum whole | whole cohort | grouped / subsets",
              flush=True)
    for G in GS:
        for kind in ("random", "contiguous"):
            lab = labels(nn, G, kind)
            groups = capi.SampleGroups(lab, G)
            ssets = [capi.SampleSet(lab == k) for k in range(G)] if fmt == capi.FMT_DS32 else []
            grp, sub, one = [], [], []
            for _ in range(reps):
                grp.append(timed(sc, lambda: sc.score_cohort_def_groups(co, sd, groups)))
                if ssets:
                    sub.append(sum(timed(sc, lambda s=s: sc.score_cohort_def_subset(co, sd, s)) for s in ssets))
                try:
                    one.append(timed(sc, lambda: sc.score_cohort_def(co, sd, 0, whole_mode)))
                except capi.NpsError:   # (a DS16 shape the single-read grid does not fit: no whole-cohort figure)
                    one.append(np.full(3, np.nan))
            g, w = best(grp), best(one)
            s = best(sub) if sub else np.array([np.nan, np.nan, subset_of[(G, kind)]])
            out[(G, kind)] = s[2]
            if not quiet:
                print("%s %d %-10s | %8.2f %8.2f %8.2f | %8.2f %8.2f %8.2f | %8.2f | %.3f"
                      % (name, G, kind, g[0], g[1], g[2], s[0], s[1], s[2], w[2], g[2] / s[2]), flush=True)
            for x in [groups] + ssets:
                x.close()
    for x in (sc, sd, co):
        x.close()
    return out


warm = case("warm-up", capi.FMT_DS32, 30_000, 512, 1, quiet=True)   # every kernel once
case("warm-up", capi.FMT_DS16, 30_000, 512, 1, subset_of=warm, quiet=True)
ds32 = case("DS32", capi.FMT_DS32, a.samples, m, a.reps)
case("DS16", capi.FMT_DS16, a.samples, m, a.reps, subset_of=ds32)
