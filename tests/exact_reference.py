"""References finer than the oracle, and the error bar each scoring path's own arithmetic implies (not a conftest:
imported by tests/test_exact_reference.py and tests/test_gpu_exact.py).

* `impute` restates getImputedDosages (nimpress.nim:484-585) over whole rows: the dosage every used row gives every
  sample, as the reference's own doubles (2 eaf, neffect / ngenotyped as an IEEE division, 0 / 2 for hom-ref).
* Exact designs (`exact_design`): betas k 2^-q, eafs j / 2^p, and every row whose missing samples are imputed from its
  own tally has a power-of-two genotyped count.  Every term and partial sum is then an integer multiple of one power of
  two below 2^53: `integer_reference` sums them in int64 and divides by 2 nloci and adds the offset as the reference
  does.  On such a definition every path that adds exactly, and the oracle, must give the same bits.
* `dd_reference`: realistic inputs.  Each dosage * beta exactly (Dekker TwoProduct), summed with TwoSum over the rows,
  vectorised over the samples; the pair (hi, lo) is within n^2 2^-106 sum |t| of the exact sum.
* `strip_mirror`: a numpy model of the fixed-point strip kernels (nps_mx.hip, nps_mxg.hip) with switches for the faults
  the bars must catch.
* `strip_bound` / `f64_bound`: the per-sample bars of section "Numerics" in DESIGN.md.
"""
import math

import numpy as np

U = 2.0 ** -53                     # unit roundoff of float64
LOCUS = {"ps": 0, "homref": 1, "fail": 2, "ignore": 3}
SAMPLE_INTERNAL = ("int_ps", "int_fail")
CODE_DOSAGE = np.array([0.0, 1.0, np.nan, 2.0])   # 2-bit codes (tests/special_cases.py): 2 = missing
FLUSH_SB = 1024                    # kFlushSb, nps_mx_route.h
BAND_BITS, MAX_BANDS = 30, 8       # kMxBandBits, kMxMaxBands, nps_scale.h


def gamma(k):
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------------------------------------------------------
# the reference's row loop, over whole rows
def impute(dos, beta, eaf, rie, params, kind=None):
    """dos: [m, n] raw dosages (NaN = missing) of the PRESENT rows, in order.  Returns (D, used, over, rows) with D the
    [r, n] dosages of the r used rows (rows: their indices among the descriptors), over[r] True where the row is a locus
    imputation over --maxmis (a constant the strip kernels add apart, as `s_const`)."""
    n = dos.shape[1]
    m = beta.size
    kind = np.zeros(m, np.int32) if kind is None else np.asarray(kind)
    out, rows, over = [], [], []
    r = 0

    def locus(j):
        il = params["imp_locus"]
        if il == "ignore":
            return None
        v = 2.0 * eaf[j] if il == "ps" else ((2.0 if rie[j] else 0.0) if il == "homref" else np.nan)
        return np.full(n, v)

    for j in range(m):
        k = int(kind[j])
        if k in (1, 3):                            # uncovered, filtered (nimpress.nim:526-531, 553-558)
            d, ov = locus(j), True
        elif k == 2:                               # absent (:536-551)
            d, ov = (np.full(n, 2.0 if rie[j] else 0.0) if params["imp_missing"] == "homref" else None), True
        else:
            x = dos[r].astype(np.float64)
            r += 1
            miss = np.isnan(x)
            nm = float(miss.sum())
            ng = float(n) - nm
            ne = float(np.sum(x[~miss]))
            if nm / float(n) > params["maxmis"]:  # :565-571
                d, ov = locus(j), True
            else:
                s = params["imp_sample"]
                if s == "ps":
                    v = 2.0 * eaf[j]
                elif s == "homref":
                    v = 2.0 if rie[j] else 0.0
                elif s == "fail":
                    v = np.nan
                elif ng >= params["mincs"]:
                    v = ne / ng
                else:
                    v = 2.0 * eaf[j] if s == "int_ps" else np.nan
                d, ov = np.where(miss, v, x), False
        if d is not None:
            out.append(d)
            rows.append(j)
            over.append(ov)
    D = np.array(out).reshape(len(out), n)
    return D, np.array(rows, dtype=np.int64), np.array(over, dtype=bool)


def codes_dosages(codes):
    return CODE_DOSAGE[codes]


def unpack(packed, n):
    """[rows, words] uint32 -> [rows, n] 2-bit codes (tests/special_cases.py pack, inverted)"""
    sh = (np.arange(16, dtype=np.uint32) * 2)[None, None, :]
    return ((np.asarray(packed, np.uint32)[:, :, None] >> sh) & 3).reshape(packed.shape[0], -1)[:, :n].astype(np.uint8)


def finish(sums, nloci, offset):
    """nimpress.nim:643-649 on un-normalised sums (float64, the reference's two operations)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.asarray(sums, np.float64) / (float(nloci) * 2.0) + offset


# ------------------------------------------------------------------------------------------------------------------
# integer reference (exact designs)
def dyadic_exponent(x):
    """the least e >= 0 with x 2^e an integer, for finite dyadic x (asserted)"""
    x = np.unique(np.asarray(x, np.float64))
    x = x[np.isfinite(x) & (x != 0)]
    if x.size == 0:
        return 0
    m, e = np.frexp(x)                        # x = m 2^e, m in [0.5, 1): m 2^53 is an integer
    mi = (m * 2.0 ** 53).astype(np.int64)
    tz = np.zeros(mi.size, np.int64)
    v = np.abs(mi)
    for b in range(53):
        low = (v >> b) & 1
        tz = np.where((tz == b) & (low == 0), b + 1, tz)
    need = 53 - tz - e
    return int(max(0, need.max()))


def integer_reference(dos, beta, eaf, rie, params, offset, kind=None):
    """scores of an exact design: the sum of the terms in int64 (one power-of-two unit), then / (2 nloci) + offset.
    Returns (scores, nloci, sums)."""
    D, rows, _ = impute(dos, beta, eaf, rie, params, kind)
    n = dos.shape[1]
    if rows.size == 0:
        return finish(np.zeros(n), 0, offset), 0, np.zeros(n)
    b = beta[rows]
    nan = np.isnan(D).any(axis=0) | np.isnan(b).any()
    Dz = np.where(np.isnan(D), 0.0, D)
    ed, eb = dyadic_exponent(Dz), dyadic_exponent(b)
    Di, bi = Dz * 2.0 ** ed, b * 2.0 ** eb
    assert np.all(Di == np.round(Di)) and np.all(bi == np.round(bi)), "not an exact design"
    assert np.abs(Di).max() * np.abs(bi).sum() < 2.0 ** 62, "int64 sums would overflow"
    S = Di.astype(np.int64).T @ bi.astype(np.int64)            # exact
    assert np.abs(S).max() < 2 ** 53, "the sums are not exact doubles: not an exact design"
    sums = S.astype(np.float64) * 2.0 ** -(ed + eb)
    sums[nan] = np.nan
    return finish(sums, rows.size, offset), int(rows.size), sums


def exact_design(n, m, seed, q=12, kmax=1024, p=4, rie_every=4, over=True):
    """2-bit codes and a definition on one dyadic grid: beta = k 2^-q (|k| <= kmax), eaf = j / 2^p.  Row j has no
    missing sample (j % 3 == 0), n - 2^t missing (j % 3 == 1; 2^t the largest power of two below n) or, with `over`,
    n - 2^(t-1) (j % 3 == 2: over any --maxmis below a half): every genotyped count a row can impute from is a power of
    two.  Missing genotypes fall on the first n - 2^(t-1) samples only, so that the others keep a finite score under
    --imputesample fail."""
    rng = np.random.default_rng(seed)
    codes = rng.choice(np.array([0, 1, 3], np.uint8), size=(m, n), p=[0.45, 0.4, 0.15])
    t = max(0, int(math.floor(math.log2(max(n - 1, 1)))))
    for j in range(m):
        ng = n if j % 3 == 0 or (j % 3 == 2 and not over) else (2 ** t if j % 3 == 1 else 2 ** max(t - 1, 0))
        if ng < n:
            codes[j, rng.choice(n - 2 ** max(t - 1, 0), n - ng, replace=False)] = 2
    beta = rng.integers(-kmax, kmax + 1, m) * 2.0 ** -q
    eaf = rng.integers(1, 2 ** p, m) / 2.0 ** p
    rie = (np.arange(m) % rie_every == 1).astype(np.int32)
    return codes, beta, eaf, rie


def two_band_design(n, m, seed):
    """an exact design whose odd rows' betas are 2^-31 of the even rows' (|k| <= 16): a weight span just over 2^30,
    two magnitude bands, every sum still an exact double"""
    codes, beta, eaf, rie = exact_design(n, m, seed, kmax=16)
    return codes, np.where(np.arange(m) % 2 == 0, beta, beta * 2.0 ** -31), eaf, rie


# ------------------------------------------------------------------------------------------------------------------
# double-double reference (realistic inputs)
_SPLIT = 134217729.0   # 2^27 + 1


def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def two_prod(a, b):
    """a b = p + e exactly (Dekker; no overflow in the split for |a|, |b| < 2^996)"""
    p = a * b
    ca, cb = _SPLIT * a, _SPLIT * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def dd_sum(D, b):
    """sum_j D[j, i] b[j] for every sample i as a double-double (hi, lo), and sum_j |D[j, i] b[j]|"""
    n = D.shape[1]
    hi, lo, ab = np.zeros(n), np.zeros(n), np.zeros(n)
    for j in range(D.shape[0]):
        p, e = two_prod(D[j], b[j])
        hi, s = two_sum(hi, p)
        lo = lo + (s + e)
        ab = ab + np.abs(p)
    hi, lo = two_sum(hi, lo)
    return hi, lo, ab


def dd_reference(dos, beta, eaf, rie, params, kind=None):
    """(hi, lo, sum |t|, nloci, D, b, over): the sums of the used rows' terms, in double-double"""
    D, rows, over = impute(dos, beta, eaf, rie, params, kind)
    b = beta[rows]
    hi, lo, ab = dd_sum(D, b) if rows.size else (np.zeros(dos.shape[1]),) * 3
    return hi, lo, ab, int(rows.size), D, b, over


def sum_error(got, nloci, hi, lo):
    """|got * 2 nloci - (hi + lo)| for finite samples (got: normalised scores with offset 0), in double-double"""
    p, e = two_prod(np.asarray(got, np.float64), float(2 * nloci))
    d1, d2 = two_sum(p, -hi)
    return np.abs(d1 + (d2 + (e - lo)))


# ------------------------------------------------------------------------------------------------------------------
# bars.  Each returns, per sample, the largest |got 2 nloci - exact sum| the path's arithmetic can produce (got with
# offset 0); the division by 2 nloci adds u |got 2 nloci| (one rounding, nimpress.nim:646).
def f64_bound(ab, m_used, got, nloci):
    """row layout gt2_*, streaming push_*, DS ds32_* / ds16_*, partial_shards_gt2: every term fl(d beta) (1 rounding; a
    precomputed 4-genotype LUT entry, nps_kernels.hip / nps_fused.hip, is that same one product), then any summation
    tree of the m used rows' terms -- lane sums, team partials, chunk sums, the fold -- has at most m - 1 additions on a
    path, and the int_ps value neffect / ngenotyped differs from the IEEE quotient by at most 2 ulps where a kernel
    divides with a reciprocal: gamma_(m + 2) sum |t| (Higham, Accuracy and Stability, 4.2)"""
    return gamma(m_used + 2) * ab + U * np.abs(got) * 2 * nloci * (1 + 2 * U)


def strip_scale(beta, eaf):
    """F of the fixed-point pass: bound = max |beta| (4 + max(2, 2 |eaf|)) < 2^e2, F = 56 - e2 (nps_scale.h:
    mx_scale_exponent of the bound mx_special gives a row)"""
    ie = np.maximum(2.0, 2.0 * np.abs(eaf))
    bound = float(np.max(np.abs(beta) * (4.0 + ie))) if beta.size else 0.0
    if bound <= 0.0:
        return 56
    return min(1000, max(-1000, 56 - math.frexp(bound)[1]))


def strip_bands(beta, eaf):
    """band of every row (0 for a zero beta) and the scale of every band, as nps_scoredef_create makes them
    (nps_scale.h: mx_band_plan; tests/test_weight_scale.py holds the two to each other)"""
    ie = np.maximum(2.0, 2.0 * np.abs(eaf))
    v = np.abs(beta) * (4.0 + ie)
    if not (v > 0).any():
        return np.zeros(beta.size, np.int64), [56]
    e_top = math.frexp(float(v.max()))[1]
    band = np.zeros(beta.size, np.int64)
    nz = v > 0
    band[nz] = np.clip((e_top - np.frexp(v[nz])[1]) // BAND_BITS, 0, MAX_BANDS - 1)
    F = []
    for b in range(int(band.max()) + 1):
        sel = nz & (band == b)
        F.append(strip_scale(beta[sel], eaf[sel]) if sel.any() else None)
    return band, F


def strip_bound(D, b, eaf, over, genotyped, ab, got, nloci, n_bands_used=None):
    """strip kernels gt2x_* / partial_gt2x, per sample, in units of the score sum:
    * a genotyped term g w1 2^-F with w1 = rn(beta 2^F) (nps_mx.hip:67): g / 2 units of 2^-F;
    * an imputed term: the kernel's weight rn(fl(imp' w1)) (nps_mx_common.h:166-170) with imp' = fast_ratio, within an
      ulp of the IEEE quotient (nps_mx_common.h:101): 1/2 (rounding to an integer) + imp / 2 (w1's own rounding, times
      imp) + 3 u |imp w1| (the ulp of imp' and the product's rounding); the fall-back weight rn(fl(imp beta) 2^F)
      (nps_mx.hip:77): 1/2 + u |imp beta| 2^F -- both below 1/2 + |imp| / 2 + 4 u |imp beta| 2^F;
    * the digit sums are exact, hi / lo exact in int64, and (double)hi 2^28 + (double)lo is one rounding, so is
      + s_const, and every further band's add into the partial scores (nps_mx.hip:602-607): 2 n_bands - 1 roundings of
      at most u (sum |t| + bar);
    * s_const: the over-maxmis rows' fl(c beta) (nps_mx_common.h:140) added in some order: gamma_(rows) sum |c beta|."""
    band, F = strip_bands(b, eaf)
    nb = len([f for f in F if f is not None]) if n_bands_used is None else n_bands_used
    unit = np.array([2.0 ** -F[k] if F[k] is not None else 0.0 for k in band])
    Dz = np.where(np.isnan(D), 0.0, D)
    q = np.where(genotyped, np.abs(Dz) / 2.0, 0.5 + np.abs(Dz) / 2.0 + 4 * U * np.abs(Dz * b[:, None]) / unit[:, None])
    q = np.where(b[:, None] == 0, 0.0, q)
    quant = (np.where(over[:, None], 0.0, q) * unit[:, None]).sum(axis=0)
    cst = (np.abs(Dz * b[:, None]) * over[:, None]).sum(axis=0)
    r = (2 * nb - 1) * U * (ab + quant) * (1 + 4 * U)
    return quant * (1 + 4 * U) + r + gamma(int(over.sum()) + 1) * cst + U * np.abs(got) * 2 * nloci * (1 + 2 * U)


# ------------------------------------------------------------------------------------------------------------------
# numpy mirror of the strip formulation (nps_mx.hip, nps_mx_common.h)
MUTATIONS = ["none"] + ["drop%d" % k for k in range(1, 14)] + [
    "window_x2", "sign_lost", "fold_shift", "imp_float32", "band_scale"]


def rn_int(x):
    """__double2ll_rn: round half to even; exact for |x| < 2^63 (np.rint on float64, then int)"""
    return np.rint(x).astype(np.int64)


def fast_ratio(nv, d):
    """the kernel's Newton-Raphson quotient, modelled as the IEEE one (the bar allows an ulp either way)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return nv / d


def sm_digits(w):
    """mx_codes (nps_mx_common.h:76): fourteen hexadecimal digits of |w| with the sign of w, [.., 14] int64"""
    aw = np.abs(w)
    sh = (np.arange(14, dtype=np.int64) * 4)
    dig = (aw[..., None] >> sh) & 15
    return np.where(w[..., None] < 0, -dig, dig)


def strip_weights(codes, beta, eaf, rie, params, F, mutation="none"):
    """per used PRESENT row: the integer weight of a unit of dosage w1 and the weight wi of a missing genotype, as
    mx_prep_kernel / mx_row make them (nps_mx.hip:46-80, nps_mx_common.h:116-184); rows over --maxmis: None (their
    constant is s_const).  Returns (rows, w1, wi, const_products, over_rows, nloci)."""
    n = codes.shape[1]
    scale = 2.0 ** F
    w1 = rn_int(beta * scale)
    miss = codes == 2
    nm = miss.sum(axis=1).astype(np.float64)
    ng = n - nm
    ne = np.where(miss, 0, np.array([0, 1, 0, 2])[codes]).sum(axis=1).astype(np.float64)
    over = nm / float(n) > params["maxmis"]
    il, s = params["imp_locus"], params["imp_sample"]
    homv = np.where(rie != 0, 2.0, 0.0)
    if s == "homref":
        fb = homv
    elif s in ("fail", "int_fail"):
        fb = np.full(beta.size, np.nan)
    else:
        fb = 2.0 * eaf
    with np.errstate(invalid="ignore"):
        t = fb * beta
    wfb = np.where(np.isfinite(t), np.rint(np.where(np.isfinite(t), t, 0.0) * scale), 0).astype(np.int64)
    wfb_bad = ~np.isfinite(t)
    internal = s in SAMPLE_INTERNAL
    use_int = internal & (ng >= params["mincs"])
    imp = fast_ratio(ne, ng)
    if mutation == "imp_float32":
        imp = imp.astype(np.float32).astype(np.float64)
    imp_nan = np.isnan(imp)
    wint = rn_int(np.where(imp_nan, 0.0, imp) * w1.astype(np.float64))
    wi = np.where(use_int, np.where(imp_nan, 3 * w1, wint), wfb)
    bad = np.where(use_int, imp_nan, wfb_bad)
    cv = 2.0 * eaf if il == "ps" else (homv if il == "homref" else np.full(beta.size, np.nan))
    used = np.where(over, il != "ignore", True)
    return w1, wi, bad, over, cv * beta, used


def strip_mirror(codes, beta, eaf, rie, params, offset=0.0, mutation="none", Q=1, flush_sb=FLUSH_SB):
    """scores as the strip kernels make them, for the PRESENT rows of `codes` ([m, n] 2-bit codes), one pass per
    magnitude band.  Column sums: per superblock of 128 rows one exact MFMA product added to the float32 accumulator,
    which is written out and zeroed every `flush_sb` superblocks of a team (nps_mx.hip store_c / kFlushSb)."""
    m, n = codes.shape
    band, Fb = strip_bands(beta, eaf)
    if mutation == "window_x2":
        flush_sb = 2 * flush_sb
    part = np.zeros(n)
    nloci = 0
    isnan = np.zeros(n, bool)
    for bnd, F in enumerate(Fb):
        if F is None:
            continue
        bb = np.where(band == bnd, beta, 0.0)
        w1, wi, bad, over, cb, used = strip_weights(codes, bb, eaf, rie, params, F, mutation)
        if bnd == 0:
            nloci = int(used.sum())
        g = np.array([0, 1, 3, 2])[codes]                      # GT2X codes: dosage, 3 = missing
        odd = (np.arange(n) & 1).astype(bool)
        ok = ~over
        # the two operands per row: code x digits(w1) and is_missing x digits(wi - c w1), c = 3 (even) / 4 (odd)
        dw1 = sm_digits(w1)
        if mutation == "sign_lost":
            dw1[:, 5] = np.abs(dw1[:, 5])
        sb_rows = 128
        n_sb = (m + sb_rows - 1) // sb_rows
        acc = np.zeros((Q, n, 14), np.float32)
        cnt = np.zeros(Q, np.int64)
        hi = np.zeros(n, np.int64)
        lo = np.zeros(n, np.int64)
        shift = 4 * 7 if mutation != "fold_shift" else 4 * 8

        def flush(tm):
            nonlocal hi, lo
            a = acc[tm].astype(np.int64)
            lo += sum(a[:, d] << (4 * d) for d in range(7))
            hi += sum(a[:, d + 7] << (4 * d) for d in range(7))
            acc[tm] = 0

        de = sm_digits(wi - 3 * w1)
        do = sm_digits(wi - 4 * w1)
        for k in range(n_sb):
            tm = k % Q
            r = slice(k * sb_rows, min(m, (k + 1) * sb_rows))
            gk = np.where(ok[r, None], g[r], 0)
            mk = (gk == 3)
            code = np.where(mk & odd[None, :], 4, gk)
            bc = code.T.astype(np.int64) @ (dw1[r] * ok[r, None])
            bm = (mk & ~odd[None, :]).T.astype(np.int64) @ (de[r] * ok[r, None])
            bm += (mk & odd[None, :]).T.astype(np.int64) @ (do[r] * ok[r, None])
            if mutation.startswith("drop"):
                bc[:, : int(mutation[4:])] = 0
                bm[:, : int(mutation[4:])] = 0
            isnan |= (mk & (bad[r] & ok[r])[:, None]).any(axis=0)
            # two MFMAs per superblock into the float32 accumulator: each product exact, each add one float32 rounding
            acc[tm] = acc[tm] + bc.astype(np.float32)
            acc[tm] = acc[tm] + bm.astype(np.float32)
            cnt[tm] += 1
            if cnt[tm] % flush_sb == 0:
                flush(tm)
        for tm in range(Q):
            if cnt[tm] % flush_sb:
                flush(tm)
        total = hi.astype(np.float64) * float(1 << shift) + lo.astype(np.float64)
        with np.errstate(invalid="ignore"):
            s_const = float(np.sum(cb[over & used]))
        r = total * 2.0 ** -(F + (1 if mutation == "band_scale" and bnd == 1 else 0)) + s_const
        part = r if bnd == 0 else part + r
    with np.errstate(invalid="ignore"):
        part = np.where(isnan, np.nan, part)
    return finish(part, nloci, offset), nloci


# ------------------------------------------------------------------------------------------------------------------
# digit probes: integer weights that fill all fourteen hexadecimal digits
def probe_betas(m, seed, F=56, top=-4):
    """full-mantissa betas in the top binade [2^top, 2^(top+1)) of a definition whose F is 56 - (top + 4) (eafs <= 1:
    bound = 6 max |beta| < 2^(top + 4)); beta 2^F is an integer of 53 bits, digits 0 .. 13"""
    rng = np.random.default_rng(seed)
    mant = rng.integers(0, 2 ** 52, m, dtype=np.int64) + 2 ** 52          # 53-bit odd-or-even mantissas
    sign = np.where(rng.uniform(size=m) < 0.5, -1, 1)
    return sign * np.ldexp(mant.astype(np.float64), top - 52)


def int_dot(G, W, split=28):
    """sum_j G[j, i] W[j] exactly for int64 G (small) and W (|W| < 2^62), as int64 halves (hi, lo):
    sum = hi 2^split + lo"""
    G = np.asarray(G, np.int64)
    W = np.asarray(W, np.int64)
    wh, wl = W >> split, W & ((1 << split) - 1)
    return G.T @ wh, G.T @ wl


def int_to_double(hi, lo, split=28):
    """correctly rounded hi 2^split + lo (|hi|, |lo| < 2^53: both exact doubles, one rounding in the add)"""
    assert np.abs(hi).max(initial=0) < 2 ** 53 and np.abs(lo).max(initial=0) < 2 ** 53
    return hi.astype(np.float64) * float(1 << split) + lo.astype(np.float64)


def probe_reference(codes, beta, eaf, rie, F, offset=0.0):
    """the exact score of a digit-probe design under --imputesample homref (missing -> 0 or 2): the integer sum of
    g rn(beta 2^F), correctly rounded once, then scaled, / 2 nloci + offset (the strip kernels' own order of
    operations after their exact fold)"""
    w1 = rn_int(beta * 2.0 ** F)
    assert np.all(w1.astype(np.float64) == beta * 2.0 ** F), "beta 2^F must be an integer"
    g = np.array([0, 1, 0, 2])[codes].astype(np.int64)
    g = np.where(codes == 2, np.where(rie[:, None] != 0, 2, 0), g)
    hi, lo = int_dot(g, w1)
    return finish(int_to_double(hi, lo) * 2.0 ** -F, beta.size, offset)


def ulps_apart(a, b):
    """|a - b| in ulps of b (finite values of one sign)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.spacing(np.abs(b))


SAT_PARAMS = dict(imp_locus="ps", imp_missing="homref", imp_sample="ps", maxmis=1.0, mincs=0)
SAT_EAF = 10.0   # imputed dosage 20: a missing genotype weighs 20 w1 = 16 w1 + 4 w1 (exact: 5 w1 < 2^53)
SAT_F = 60


def saturation_design(n, n_sb, seed):
    """codes periodic in 128 rows (one block [128, n]), n_sb superblocks of non-periodic weights that saturate the
    digit columns of the strip kernels: w1 = 0x5FFFFFFFFFFFF - r 16^10 (digits 0 .. 9 and 11 are 15, digit 10 is 15 or 14),
    eaf 10 under --imputesample ps.  A sample missing in every row (i % 4 == 1, an odd sample) adds, per row, 4 d_k(w1)
    for its code 4 plus d_(k-1)(w1) for 20 w1 - 4 w1 = 16 w1 to digit column k: 75 (column 11: 75 or 74, so that a
    rounded float32 sum in it shows in the score's double), 9.8e6 > 2^23 per flush
    window of 1024 superblocks, and more than 2^24 in a window twice as long, with odd sums in some superblocks.
    Returns (block codes, beta, eaf, rie)."""
    rng = np.random.default_rng(seed)
    block = rng.choice(np.array([0, 1, 3, 2], np.uint8), size=(128, n), p=[0.4, 0.35, 0.2, 0.05])
    block[:, 1::4] = 2
    m = 128 * n_sb
    w1 = 0x5FFFFFFFFFFFF - rng.integers(0, 2, m, dtype=np.int64) * 16 ** 10
    beta = np.ldexp(w1.astype(np.float64), -SAT_F)
    eaf = np.full(m, SAT_EAF)
    assert strip_scale(beta, eaf) == SAT_F and len(strip_bands(beta, eaf)[1]) == 1
    return block, beta, eaf, np.zeros(m, np.int32)


def saturation_reference(block, beta, offset=0.0):
    """the exact scores of a saturation design: per residue r of the 128-row period the sum W_r of its rows' w1, then
    sum_r c_ir W_r with c = dosage, or 20 for a missing genotype -- exact in int64 halves, rounded once"""
    w1 = rn_int(beta * 2.0 ** SAT_F)
    m = w1.size
    W = w1.reshape(m // 128, 128).sum(axis=0)                      # < 1025 x 2^51: int64
    c = np.array([0, 1, int(2 * SAT_EAF), 2])[block].astype(np.int64)
    hi, lo = int_dot(c, W)
    return finish(int_to_double(hi, lo) * 2.0 ** -SAT_F, m, offset)


def column_peak(block, beta, samples, flush_sb=FLUSH_SB, Q=1):
    """the largest |digit-column sum| within one flush window over the given samples (mirror of the accumulation,
    integer), with the superblocks dealt to Q row teams (superblock k to team k % Q, a window = flush_sb superblocks of
    one team): how close the design comes to float32's 2^24"""
    w1 = rn_int(beta * 2.0 ** SAT_F)
    code = np.array([0, 1, 3, 2])[block[:, samples]]
    odd = (np.asarray(samples) & 1).astype(bool)
    c = np.where(code == 3, np.where(odd, 4, 3), code)
    mk = code == 3
    n_sb = w1.size // 128
    blk = np.zeros((n_sb, len(samples), 14), np.int64)
    for k in range(n_sb):
        w = w1[k * 128:(k + 1) * 128]
        blk[k] = c.T @ sm_digits(w) + (mk & ~odd).T @ sm_digits(20 * w - 3 * w) + (mk & odd).T @ sm_digits(20 * w - 4 * w)
    peak = 0
    for tm in range(Q):
        mine = blk[tm::Q]
        for k0 in range(0, mine.shape[0], flush_sb):
            peak = max(peak, int(np.abs(mine[k0:k0 + flush_sb].sum(axis=0)).max()))
    return peak


def given_teams(n_strips, cus, n_sb):
    """row teams of the given-tallies plan (mx_plan_for with two_pass, nps_mx_route.h;
    tests/test_mx_route.py holds the two together): of the team counts that give 2 to
    8 rounds of the grid, the one whose last round is fullest"""
    lo = max(1, (2 * cus + n_strips - 1) // n_strips)
    hi = max(lo, 8 * cus // n_strips)
    best, q = -1.0, lo
    for t in range(lo, hi + 1):
        wg = n_strips * t
        fill = wg / (((wg + cus - 1) // cus) * cus)
        if fill > best + 1e-9:
            best, q = fill, t
    return max(1, min(q, n_sb))


# ------------------------------------------------------------------------------------------------------------------
# digit probes over several magnitude bands, and under int_ps
def banded_probe_betas(m, n_bands, seed, top=-4):
    """row j in band j % n_bands: full-mantissa betas in the binade [2^t_b, 2^(t_b + 1)), t_b = top - 30 b - 2 b (a
    bound exponent 30 b + 1 .. 30 b + 3 below the top one: band b exactly, nps_scale.h: mx_band_plan)"""
    rng = np.random.default_rng(seed)
    mant = rng.integers(0, 2 ** 52, m, dtype=np.int64) + 2 ** 52
    sign = np.where(rng.uniform(size=m) < 0.5, -1, 1)
    b = np.arange(m) % n_bands
    return sign * np.ldexp(mant.astype(np.float64), top - 32 * b - 52)


def banded_probe_reference(codes, beta, eaf, rie, params, offset=0.0):
    """the strip kernels' result on a probe design, formed as they form it: per band the exact integer sum of its
    weights (g w1 for a genotype, the imputed weight for a missing one: 0 / 2 w1 under homref, rn(fl(imp w1)) under
    int_ps with an exact power-of-two ratio), rounded once and scaled by 2^-F_b; the bands added in order into the
    partial scores (nps_mx.hip:604-607); / 2 nloci + offset.  No row may be over --maxmis."""
    band, Fb = strip_bands(beta, eaf)
    g = np.array([0, 1, 0, 2])[codes].astype(np.int64)
    miss = codes == 2
    n = codes.shape[1]
    ng = n - miss.sum(axis=1)
    ne = np.where(miss, 0, g).sum(axis=1)
    assert not np.any(miss.sum(axis=1) / float(n) > params["maxmis"])
    part = None
    for b, F in enumerate(Fb):
        if F is None:
            continue
        sel = band == b
        w1 = rn_int(np.where(sel, beta, 0.0) * 2.0 ** F)
        assert np.all(w1[sel].astype(np.float64) == beta[sel] * 2.0 ** F)
        if params["imp_sample"] == "homref":
            wi = np.where(rie != 0, 2 * w1, 0)
        else:
            assert params["imp_sample"] == "int_ps" and params["mincs"] <= ng.min()
            assert np.all((ng & (ng - 1)) == 0) or np.all(miss.sum(axis=1)[ng & (ng - 1) != 0] == 0)
            wi = rn_int((ne / ng) * w1.astype(np.float64))        # fast_ratio is exact for a power-of-two count
        G = np.where(miss, 0, g)
        hi, lo = int_dot(G, w1)
        mh, ml = int_dot(miss.astype(np.int64), wi)
        r = int_to_double(hi + mh + ((lo + ml) >> 28), (lo + ml) & ((1 << 28) - 1)) * 2.0 ** -F
        part = r if part is None else part + r
    return finish(part, beta.size, offset)


# ------------------------------------------------------------------------------------------------------------------
# the multi-score path (nps_multi.hip)
def multi_scale(beta, eaf, ND):
    """F[s] = 8 ND - 9 - e, bound = max |beta| (3 + max(2, 2 max |eaf|)) < 2^e (nps_scale.h: multi_scale)"""
    bound = float(np.max(np.abs(beta))) * (3.0 + max(2.0, 2.0 * float(np.max(np.abs(eaf)))))
    return 8 * ND - 9 - (math.frexp(bound)[1] if bound > 0 else 0), bound


def multi_bound(D, b, eaf, over, genotyped, ab, got, nloci, ND, missing_bits=56, beta_all=None, n_missing=None):
    """multi-score pass, per sample, on the un-normalised sum:
    * dosage weights VD = llrint(beta 2^F) (nps_multi.hip:400): g / 2 units of 2^-F for a genotype g;
    * a missing genotype: 3 VD from its code plus VM = llrint(fl(fl(imp beta) - fl(3 beta)) 2^F) (nps_multi.hip:391,
      401): 3/2 + 1/2 units and u (2 |imp beta| + 6 |beta|) for the three float64 roundings; with 40 / 32-bit missing
      weights the coarse truncation adds 2^-32 B / 2^-24 B per missing genotype of the sample in ANY present row
      (include/nps.h:385-393, B = max |beta| (3 + max(2, 2 max eaf))): the rounded prefix coefficients mix the weights of
      four rows, so a genotype missing in a row over --maxmis, whose own weight is zero, still meets rounded ones;
    * the constants: fl(c beta) (u |c beta|), llrint (1/2 unit each), an exact int sum, ldexp (one rounding of the total)
      and the add to the running constant (nps_multi.hip:676-677);
    * the digit sums are exact in int64, Horner in float64 (nps_multi.hip:700) has ND adds whose roundings are at most
      u of a prefix sum, i.e. of sum |t| plus the signed low digits still outside it: below 2^(8 (ND-1) - 1) units per
      coefficient, four coefficients per row; then + constants (one rounding) and / 2 nloci."""
    beta_all = b if beta_all is None else beta_all
    F, B = multi_scale(beta_all, eaf, ND)
    unit = 2.0 ** -F
    Dz = np.where(np.isnan(D), 0.0, D)
    bb = np.abs(b)[:, None]
    q = np.where(genotyped, np.abs(Dz) / 2.0 * unit, 2.0 * unit + U * (2 * np.abs(Dz) * bb + 6 * bb) * (1 + 2 * U))
    q = np.where(b[:, None] == 0, 0.0, q)
    cst = np.abs(Dz * bb) * over[:, None]
    quant = (np.where(over[:, None], U * cst + unit / 2, q)).sum(axis=0)
    if missing_bits != 56:
        quant = quant + n_missing * 2.0 ** -(missing_bits - 8) * B
    low = 4 * b.size * 2.0 ** (8 * (ND - 1) - 1) * 2.0 ** -(F + 7)
    r = (ND + 3) * U * (ab + quant + low) * (1 + 4 * U)
    return quant * (1 + 4 * U) + r + U * np.abs(got) * 2 * nloci * (1 + 2 * U)
