#!/usr/bin/env python3
"""Quick benchmark of the streamed FORMAT/PL path against the existing path closest to it in bytes per row.

At 500 000 samples: 2 000 rows of nps_push_pl (int16, 2 alleles: 3 values = 6 bytes per sample, 3 MB per row) and 2 000 rows
of nps_push_gt (int32 diploid: 8 bytes per sample, 4 MB per row), alternating, two runs each in ONE process after a warm-up
of both.  Both paths are a pinned copy of the caller's row plus one kernel that reads the slot over PCIe.  Printed per run:
rows/s and host-to-device GB/s over the wall time from the first push to the return of Scorer.sync() -- nps_flush with no
statistics buffer, which completes every pushed row (host clock around work that ends in a synchronise; the scoring kernels
of the rows are inside it), and the decode kernels' own time from HIP events
(nps_profile: ms_decode) in a separate run, since the events slow the host.

    python tools/qb_pl.py [--samples N] [--rows M]

The bar: PL bytes/s >= 0.9 x the nps_push_gt bytes/s of the same process."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nimpress_amd import capi  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=500_000)
    ap.add_argument("--rows", type=int, default=2000)
    args = ap.parse_args(argv)
    n, m = args.samples, args.rows
    if capi.device_count() < 1:
        raise SystemExit("qb_pl: no GPU (there is no CPU path to time)")
    rng = np.random.default_rng(1)
    # eight distinct host rows of each kind, pushed in turn
    vals = np.array([0, 3, 10, 20, 30, 60, 99, 255], np.int16)
    pl_rows = []
    for _ in range(8):
        pl = vals[rng.integers(0, vals.size, size=(n, 3))]
        pl[np.arange(n), rng.integers(0, 3, size=n)] = 0
        pl[rng.uniform(size=n) < 0.02] = 0           # uninformative samples
        pl_rows.append(np.ascontiguousarray(pl))
    gt_rows = []
    for _ in range(8):
        a = rng.integers(0, 2, size=(n, 2))
        g = ((a + 1) << 1).astype(np.int32)
        g[rng.uniform(size=n) < 0.02] = 0
        gt_rows.append(np.ascontiguousarray(g))
    beta = rng.normal(0, 0.05, m)
    pl_bytes, gt_bytes = pl_rows[0].nbytes, gt_rows[0].nbytes

    def run(kind, rows, profile):
        sc = capi.Scorer(n, capi.make_params())
        if profile:
            sc.profile_enable(True)
        for j in range(8):                            # warm-up: ring, batch buffers, code object
            if kind == "pl":
                sc.push_pl(pl_rows[j], 2, 1, 0, 0.01, 0.3)
            else:
                sc.push_gt(gt_rows[j], 2, 1, 0, 0.01, 0.3)
        sc.sync()
        if profile:
            sc.profile_get(reset=True)
        t0 = time.perf_counter()
        for j in range(rows):
            if kind == "pl":
                sc.push_pl(pl_rows[j & 7], 2, 1, 0, beta[j], 0.3)
            else:
                sc.push_gt(gt_rows[j & 7], 2, 1, 0, beta[j], 0.3)
        sc.sync()
        wall = time.perf_counter() - t0
        out = dict(kind=kind, rows=rows, wall_s=wall, rows_per_s=rows / wall,
                   h2d_GBps=rows * (pl_bytes if kind == "pl" else gt_bytes) / wall / 1e9)
        if profile:
            p = sc.profile_get()
            out.update(ms_decode=p.ms_decode, n_decode=int(p.n_decode),
                       decode_us_per_row=1e3 * p.ms_decode / max(int(p.n_decode), 1),
                       decode_GBps=(pl_bytes if kind == "pl" else gt_bytes) * int(p.n_decode) / max(p.ms_decode, 1e-9) / 1e6)
        sc.close()
        return out

    print("qb_pl: %d samples, %d rows per run; PL row %d bytes (int16 x 3), GT row %d bytes (int32 x 2)" % (n, m, pl_bytes, gt_bytes))
    res = []
    for rep in range(2):
        for kind in ("pl", "gt"):
            r = run(kind, m, profile=False)
            res.append(r)
            print("run %d %-2s  %8.1f rows/s  %6.2f GB/s host-to-device  (%.3f s)" % (rep, kind, r["rows_per_s"], r["h2d_GBps"], r["wall_s"]))
    prof = {}
    for kind in ("pl", "gt"):                         # decode kernel times: a run of their own, events on
        r = run(kind, max(m // 4, 1), profile=True)
        prof[kind] = r
        print("events %-2s  decode %7.1f us per row (%d launches, %.1f ms)  = %6.2f GB/s read by the kernel" % (
            kind, r["decode_us_per_row"], r["n_decode"], r["ms_decode"], r["decode_GBps"]))
    best = {k: max(r["h2d_GBps"] for r in res if r["kind"] == k) for k in ("pl", "gt")}
    ratio = best["pl"] / best["gt"]
    print("PL %.2f GB/s, GT %.2f GB/s: ratio %.3f (bar 0.9: %s)" % (best["pl"], best["gt"], ratio, "met" if ratio >= 0.9 else "MISSED"))
    print(json.dumps(dict(samples=n, rows=m, runs=res, events=prof, pl_GBps=best["pl"], gt_GBps=best["gt"], ratio=ratio)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
