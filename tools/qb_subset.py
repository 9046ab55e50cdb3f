#!/usr/bin/env python3
"""dev tool: what does scoring a subset of a resident cohort's samples (nps_score_cohort_def_subset) cost against the
whole-cohort two-pass run (nps_score_cohort_def, NPS_MODE_TWOPASS) it is built from?  One synthetic NPS_FMT_GT2X cohort of
--samples x --variants, then one NPS_FMT_DS32 cohort of --ds-samples x --variants; for keep = all / a random half / a
contiguous tenth the two runs alternate, --reps of each, in one process on one device.  Times are HIP-event times of the
context's profile: ms_tally of the masked tally against ms_tally of the unmasked one, and the whole pass (tally + params +
accumulation + fold) against the whole two-pass run.  A small cohort is scored first with every kernel, so that no figure
holds a first launch.
    python tools/qb_subset.py [--samples 500000] [--ds-samples 200000] [--variants 100000] [--reps 3]"""
import argparse, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=500_000)
ap.add_argument("--ds-samples", type=int, default=200_000)
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


def make(fmt, nn, mm):
    co = capi.Cohort(nn, mm, fmt=fmt)
    for r0 in range(0, mm, 1 << 15):
        k = min(1 << 15, mm - r0)
        co.synth(r0, seed, th[r0:r0 + k], tm[r0:r0 + k], tmi[r0:r0 + k])
    return co


def keeps(nn):
    half = (np.random.default_rng(1).random(nn) < 0.5).astype(np.uint8)
    tenth = np.zeros(nn, np.uint8)
    tenth[nn // 3:nn // 3 + nn // 10] = 1
    return [("all", np.ones(nn, np.uint8)), ("random half", half), ("contiguous tenth", tenth)]


def timed(sc, run):
    sc.reset()
    sc.profile_enable(True)
    sc.profile_get(reset=True)
    run()
    sc.sync()
    p = sc.profile_get(reset=True)
    return p.ms_tally, p.ms_tally + p.ms_params + p.ms_accumulate + p.ms_fused + p.ms_reduce


def case(name, fmt, nn, mm, reps, quiet=False):
    co = make(fmt, nn, mm)
    sc, sd = capi.Scorer(nn, params), capi.ScoreDef(descs[:mm])
    if not quiet:
        print("# %s %d x %d" % (name, nn, mm), flush=True)
    for label, keep in keeps(nn):
        sset = capi.SampleSet(keep)
        sub, two = [], []
        for _ in range(reps):
            two.append(timed(sc, lambda: sc.score_cohort_def(co, sd, 0, capi.MODE_TWOPASS)))
            sub.append(timed(sc, lambda: sc.score_cohort_def_subset(co, sd, sset)))
        if not quiet:
            bt, bs = min(t for t, _ in two), min(t for t, _ in sub)
            wt, ws = min(w for _, w in two), min(w for _, w in sub)
            print("%s keep %-16s (%7d kept) | ms_tally masked %s, unmasked %s: best / best %.3f | whole pass subset %s, two-pass %s: "
                  "best / best %.3f" % (name, label, sset.n_kept, ", ".join("%.2f" % t for t, _ in sub),
                                        ", ".join("%.2f" % t for t, _ in two), bs / bt, ", ".join("%.2f" % w for _, w in sub),
                                        ", ".join("%.2f" % w for _, w in two), ws / wt), flush=True)
        sset.close()
    for x in (sc, sd, co):
        x.close()


for fmt in (capi.FMT_GT2X, capi.FMT_DS32):   # every kernel once
    case("warm-up", fmt, 30_000, 512, 1, quiet=True)
case("GT2X", capi.FMT_GT2X, a.samples, m, a.reps)
case("DS32", capi.FMT_DS32, a.ds_samples, m, a.reps)
