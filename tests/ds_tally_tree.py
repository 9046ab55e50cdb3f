"""The summation tree of a dosage row's tally, restated in numpy from the comment above ds_tally_kernel
(nimpress_amd/csrc/nps_ds_common.h) -- not from its code.  One 256-thread block per row:

  * a lane-of-four v holds samples 4 v .. 4 v + 3; thread t takes the lanes-of-four t, t + 256, .. in ascending order and
    the samples k = 0 .. 3 of each in order: a missing sample (NaN) counts, any other adds its float32 value as a
    float64 to the thread's float64 sum (2.0 - value to the flipped sum);
  * the wave sum as lane 0 sees it: for o = 32, 16, .. 1 lane l adds what lane l + o holds;
  * the block sum of the four waves: ((s0 + s1) + s2) + s3.

A sample dropped by the keep mask adds nothing anywhere."""
import numpy as np

THREADS, WAVE = 256, 64


def ds_tally_tree(row, keep=None):
    """row: float32[n]; keep: None or n flags.  (nmissing, sum, sum_flipped): int, float64, float64"""
    row = np.asarray(row, dtype=np.float32)
    n = row.size
    live = np.ones(n, bool) if keep is None else np.asarray(keep) != 0
    turns = max(1, -(-((n + 3) // 4) // THREADS))
    x = np.zeros(turns * THREADS * 4, np.float64)
    x[:n] = row.astype(np.float64)
    ok = np.zeros(turns * THREADS * 4, bool)
    ok[:n] = live
    x, ok = x.reshape(turns, THREADS, 4), ok.reshape(turns, THREADS, 4)
    cnt = np.zeros(THREADS, np.int64)
    s, f = np.zeros(THREADS, np.float64), np.zeros(THREADS, np.float64)
    with np.errstate(invalid="ignore"):
        for j in range(turns):
            for k in range(4):
                e, take = x[j, :, k], ok[j, :, k]
                miss = np.isnan(e)
                cnt += take & miss
                add = take & ~miss
                s = np.where(add, s + e, s)
                f = np.where(add, f + (2.0 - e), f)

    def block(v):
        waves = []
        for w in range(THREADS // WAVE):
            a = v[w * WAVE:(w + 1) * WAVE].copy()
            o = WAVE // 2
            while o:
                a = a[:o] + a[o:2 * o]
                o //= 2
            waves.append(a[0])
        return ((waves[0] + waves[1]) + waves[2]) + waves[3]

    return int(cnt.sum()), np.float64(block(s)), np.float64(block(f))
