#!/usr/bin/env python3
"""dev tool: what do S score definitions over one resident DOSAGE cohort cost in the multi-score pass (nps_score_cohort_multi:
two reads whatever S is) against S single-score passes (nps_score_cohort_def, NPS_MODE_FUSED: one read each)?  One synthetic
NPS_FMT_DS32 cohort of --samples x --variants, then the NPS_FMT_DS16 cohort of the same size; for S = 1, 2, 3, 4, 8 the two
ways alternate, --reps of each, in one process.  Times are HIP-event times of the kernels: nps_multi_timing's three figures
(tally + params, accumulation, fold) for the multi pass, the profile spans of the S passes for the yardstick.  A small cohort
is scored first with every kernel, so that no figure holds a first launch.  Prints one line per case, the share of the
8 TB/s roofline with the multi pass charged for BOTH of its reads, and the smallest S at which every multi run beat every run
of the S single passes.  Ends non-zero if any score of a multi pass is outside REL_TOL (floored) of its single-score result.
    python tools/qb_multi_ds.py [--samples 200000] [--variants 100000] [--scores 1,2,3,4,8] [--reps 2]"""
import argparse, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=200_000)
ap.add_argument("--variants", type=int, default=100_000)
ap.add_argument("--scores", default="1,2,3,4,8")
ap.add_argument("--reps", type=int, default=2)
a = ap.parse_args()
from nimpress_amd import capi
REL_TOL, HBM = 1e-7, 8e12
n, m, seed = a.samples, a.variants, 20250105
rng = np.random.default_rng(seed)
SC = 4294967296.0
f = lambda x: np.minimum(np.floor(np.asarray(x, dtype=np.float64) * SC), 4294967295.0).astype(np.uint32)
eaf_c = np.round(rng.uniform(0.01, 0.5, m), 4)
miss = rng.uniform(0, 0.08, m)
th, tm, tmi = f(eaf_c * eaf_c + 2 * eaf_c * (1 - eaf_c)), f(eaf_c * eaf_c), f(miss)
descs = np.zeros((8, m), dtype=capi.ROW_DESC_DTYPE)
for s in range(8):
    descs[s]["beta"] = np.round(rng.normal(0, 0.02 * (1 + s), m), 4)
    descs[s]["eaf"] = np.round(rng.uniform(0.01, 0.9, m), 4)
    descs[s]["ref_is_effect"] = (rng.uniform(size=m) < 0.3).astype(np.int32)
params = capi.make_params()

def rel_err(got, ref, beta_abs_sum, nloci):
    if not np.array_equal(np.isnan(got), np.isnan(ref)):
        return float("inf")
    ok = ~np.isnan(ref)
    floor = 1e-12 * beta_abs_sum / max(2.0 * nloci, 1.0)
    return float(np.max(np.abs(got[ok] - ref[ok]) / np.maximum(np.abs(ref[ok]), max(floor, 1e-300)))) if ok.any() else 0.0

def multi_pass(msc, co, mdef):
    msc.reset()
    msc.score_cohort(co, mdef)
    got, nloci = msc.finish(np.zeros(msc.n_scores))
    return msc.timing(), got.copy(), nloci

def single_passes(sc, co, sdefs):
    total, out = 0.0, []
    for sdef in sdefs:
        sc.reset()
        sc.profile_enable(True)
        sc.profile_get(reset=True)
        sc.score_cohort_def(co, sdef, 0, capi.MODE_FUSED)
        out.append(sc.finish(0.0))
        p = sc.profile_get(reset=True)
        total += p.ms_tally + p.ms_params + p.ms_accumulate + p.ms_fused + p.ms_reduce
    return total, out

def make(fmt, nn, mm):
    co = capi.Cohort(nn, mm, fmt=fmt)
    for r0 in range(0, mm, 1 << 15):
        co.synth(r0, seed, th[r0:r0 + (1 << 15)][:mm - r0], tm[r0:r0 + (1 << 15)][:mm - r0], tmi[r0:r0 + (1 << 15)][:mm - r0])
    return co

# every kernel once
for fmt in (capi.FMT_DS32, capi.FMT_DS16):
    w = make(fmt, 30_000, 512)
    ws = capi.Scorer(30_000, params)
    wd = [capi.ScoreDef(descs[0, :512])]
    single_passes(ws, w, wd)
    for S in [int(x) for x in a.scores.split(",")]:
        wm, wdef = capi.MultiScorer(30_000, params, S), capi.MultiDef(np.ascontiguousarray(descs[:S, :512]))
        multi_pass(wm, w, wdef)
        wm.close(); wdef.close()
    ws.close(); wd[0].close(); w.close()

bad, wins = 0, {}
for name, fmt, elem in (("DS32", capi.FMT_DS32, 4), ("DS16", capi.FMT_DS16, 2)):
    co = make(fmt, n, m)
    read_bytes = co.row_stride * m
    sc = capi.Scorer(n, params)
    sdefs = [capi.ScoreDef(descs[s]) for s in range(8)]
    chunks, per = capi.MultiScorer(n, params, 1).geometry(m, fmt)
    print("# %s %d x %d: %.1f GB per read, accumulation plan %d row chunks of %d rows" % (name, n, m, read_bytes / 1e9, chunks, per),
          flush=True)
    for S in [int(x) for x in a.scores.split(",")]:
        msc, mdef = capi.MultiScorer(n, params, S), capi.MultiDef(np.ascontiguousarray(descs[:S]))
        t_multi, t_single = [], []
        for rep in range(a.reps):
            (t0, t1, t2), got, nloci = multi_pass(msc, co, mdef)
            ts, one = single_passes(sc, co, sdefs[:S])
            t_multi.append((t0, t1, t2))
            t_single.append(ts)
            for s in range(S):
                e = rel_err(got[s], one[s][0], float(np.abs(descs[s]["beta"]).sum()), one[s][1])
                if int(nloci[s]) != one[s][1] or not e <= REL_TOL:
                    bad += 1
                    print("MISMATCH %s S=%d score %d: nloci %d / %d, rel. error %.3g" % (name, S, s, nloci[s], one[s][1], e), flush=True)
        tot = [sum(t) for t in t_multi]
        wins[(name, S)] = max(tot) < min(t_single)
        print("%s S=%d | multi: %s ms | %d single passes: %s ms | multi / single %.3f | multi at %.3f of the roofline (two reads), "
              "accumulation alone %.3f" % (
                  name, S, ", ".join("%.2f = %.2f tally+params + %.2f accumulate + %.2f fold" % (sum(t), *t) for t in t_multi), S,
                  ", ".join("%.2f" % t for t in t_single), min(tot) / min(t_single),
                  2 * read_bytes / HBM / (min(tot) * 1e-3), read_bytes / HBM / (min(t[1] for t in t_multi) * 1e-3)), flush=True)
        msc.close(); mdef.close()
    for x in sdefs + [sc, co]:
        x.close()
for name in ("DS32", "DS16"):
    won = [S for (nm, S), w in sorted(wins.items()) if nm == name and w]
    lost_after = [S for (nm, S), w in sorted(wins.items()) if nm == name and not w and won and S > won[0]]
    print("# %s: smallest S at which every multi run beat every run of the S single passes: %s%s" % (
        name, won[0] if won else "none", " (but not at S = %s)" % lost_after if lost_after else ""), flush=True)
sys.exit(1 if bad else 0)
