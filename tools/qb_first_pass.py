#!/usr/bin/env python3
"""dev tool: what does the FIRST NPS_MODE_AUTO pass over an UPLOADED strip cohort cost, against the later ones?  For each
cohort size: a NPS_FMT_GT2X cohort of --variants rows is filled with nps_cohort_upload from host rows (HWE genotypes from the
generator, a block of --block rows downloaded once and uploaded again and again: the kernels' time does not depend on the
genotypes), then scored --passes times; then one block is uploaded again -- a rewrite -- and the passes are repeated, --reps
times in all, so that "first pass after rows were written" is the minimum of a few like every other figure.  Prints the
upload's wall time and, per pass, the HIP-event time of its kernels, the wall time of the scoring call (a revision that counts
tallies lazily does so inside the call, outside the events) and which kernels ran.  A small cohort is scored first with every
kernel so that no figure holds a kernel's first launch.  Uses only calls every revision of the library has, so one script
measures two revisions on one box (NPS_QB_ROOT = the other revision's tree):
    python tools/qb_first_pass.py [--samples 300000,400000,1000000] [--variants 16384] [--passes 4] [--reps 3] [--label TEXT]"""
import argparse, os, sys, time
import numpy as np
ROOT = os.environ.get("NPS_QB_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--samples", default="300000,400000,1000000")
ap.add_argument("--variants", type=int, default=16384)
ap.add_argument("--block", type=int, default=2048)
ap.add_argument("--passes", type=int, default=4)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--label", default="")
a = ap.parse_args()
from nimpress_amd import capi
print("# %s  library %s" % (a.label, capi.LIB_PATH), flush=True)
m, blk, seed = a.variants, a.block, 20250103
assert blk % 128 == 0 and m % blk == 0
rng = np.random.default_rng(seed)
beta = np.round(rng.normal(0.0, 0.02, m), 4)
SC = 4294967296.0
f = lambda x: np.minimum(np.floor(np.asarray(x, dtype=np.float64) * SC), 4294967295.0).astype(np.uint32)
eaf = np.round(rng.uniform(0.01, 0.5, blk), 4)
miss = rng.uniform(0, 0.02, blk)
th, tm, tmi = f(eaf * eaf + 2 * eaf * (1 - eaf)), f(eaf * eaf), f(miss)
def one_pass(sc, co, sdef):
    sc.reset()
    sc.profile_enable(True)
    sc.profile_get(reset=True)
    t0 = time.perf_counter()
    sc.score_cohort_def(co, sdef, 0, capi.MODE_AUTO)
    sc.sync()
    wall = (time.perf_counter() - t0) * 1e3
    sc.finish(0.0)
    p = sc.profile_get(reset=True)
    kind = "+".join(k for k, c in (("tally", p.n_tally), ("in-pass", p.n_fused), ("given", p.n_accumulate)) if c)
    return p.ms_tally + p.ms_fused + p.ms_accumulate, p.ms_reduce, wall, kind
# every kernel once: the in-pass kernel, the tally kernel, the given-tallies kernel, the folds
w = capi.Cohort(270_000, 256, fmt=capi.FMT_GT2X)
w.synth(0, seed, th[:256], tm[:256], tmi[:256])
wd = capi.ScoreDef(capi.row_descs(beta[:256], 0.3 * np.ones(256)))
ws = capi.Scorer(270_000, capi.make_params())
one_pass(ws, w, wd)
w.keep_tallies()
one_pass(ws, w, wd)
ws.close(); wd.close(); w.close()
for n in [int(x) for x in a.samples.split(",")]:
    tmp = capi.Cohort(n, blk, fmt=capi.FMT_GT2X)
    tmp.synth(0, seed, th, tm, tmi)
    rows = np.ascontiguousarray(tmp.download(0, blk))
    tmp.close()
    co = capi.Cohort(n, m, fmt=capi.FMT_GT2X)
    sdef = capi.ScoreDef(capi.row_descs(beta, 0.3 * np.ones(m)))
    sc = capi.Scorer(n, capi.make_params())
    first, later, lines = [], [], []
    for rep in range(a.reps):
        t0 = time.perf_counter()
        for x in range(0, m if rep == 0 else blk, blk):   # (later reps: one block again -- a rewrite)
            co.upload(x, rows)
        if rep == 0:
            t_up = time.perf_counter() - t0
        res = [one_pass(sc, co, sdef) for _ in range(a.passes)]
        first.append(res[0])
        later += res[1:]
        lines.append(" | ".join("%.3f+%.3f ms, call %.2f ms (%s)" % r for r in res))
    f_ev, f_wall = min(r[0] for r in first), min(r[2] for r in first)
    l_ev, l_wall = min(r[0] for r in later), min(r[2] for r in later)
    print("%d x %d: upload %.3f s | first pass after a write: kernels %.3f ms, call %.2f ms | later passes: kernels %.3f ms, call %.2f ms "
          "| first / later: kernels %.3f, call %.3f" % (n, m, t_up, f_ev, f_wall, l_ev, l_wall, f_ev / l_ev, f_wall / l_wall), flush=True)
    for rep, ln in enumerate(lines):
        print("    rep %d, per pass kernels + fold, scoring call (kernels run): %s" % (rep, ln), flush=True)
    sc.close()
    sdef.close()
    co.close()
