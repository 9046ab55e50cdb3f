"""Test helper: the FORMAT/PL dosage of include/nps.h (above nps_push_pl) restated in numpy, written from the text, not from
the kernel: explicit float64 adds in ascending genotype order, one rounding per add.

    pl_dosage(pl[n, G], A, e, table) -> float32[n]

`table` is the library's nps_pl_likelihoods output (its 256 entries are checked on their own in tests/test_pl_abi.py)."""
import numpy as np

VALUES_INT8 = [0, 1, 3, 10, 30, 99, 127]
VALUES_WIDE = VALUES_INT8 + [254, 255, 256, 300, 32767]
MISSING = {np.dtype(np.int8): -128, np.dtype(np.int16): -32768, np.dtype(np.int32): -2147483648}
END_OF_VECTOR = {np.dtype(np.int8): -127, np.dtype(np.int16): -32767, np.dtype(np.int32): -2147483647}


def n_genotypes(A: int) -> int:
    return A * (A + 1) // 2


def genotypes(A: int):
    """(j, k), j <= k, in the order of the VCF specification: index k (k + 1) / 2 + j"""
    out = [(j, k) for k in range(A) for j in range(k + 1)]
    assert all(k * (k + 1) // 2 + j == g for g, (j, k) in enumerate(out))
    return out


def pl_dosage(pl, A: int, e: int, table) -> np.ndarray:
    pl = np.asarray(pl)
    G = n_genotypes(A)
    assert pl.ndim == 2 and pl.shape[1] == G and 0 <= e < A and len(table) == 256
    table = np.asarray(table, dtype=np.float64)
    p = pl.astype(np.int64)                       # sign extension from the record's width
    missing = (p < 0).any(axis=1) | (p.max(axis=1) == p.min(axis=1))
    w = table[np.clip(p, 0, 255)]                 # [n, G] float64 (negative entries only in missing samples)
    num = np.zeros(pl.shape[0], dtype=np.float64)
    den = np.zeros(pl.shape[0], dtype=np.float64)
    for g, (j, k) in enumerate(genotypes(A)):
        cnt = np.float64(int(j == e) + int(k == e))
        num = np.add(num, np.multiply(cnt, w[:, g], dtype=np.float64), dtype=np.float64)
        den = np.add(den, w[:, g], dtype=np.float64)
    out = np.divide(num, den, dtype=np.float64).astype(np.float32)
    out[missing] = np.float32("nan")
    return out


def random_pl(rng, n: int, A: int, dtype, p_bad: float = 0.12, p_flat: float = 0.06) -> np.ndarray:
    """n samples x G values drawn from the issue's value sets for the width, with typed-missing / end-of-vector values in
    about p_bad of the samples and a flat vector in about p_flat of them (so 5 % .. 40 % of the rows decode to NaN)"""
    dtype = np.dtype(dtype)
    G = n_genotypes(A)
    vals = np.array(VALUES_INT8 if dtype == np.int8 else VALUES_WIDE, dtype=np.int64)
    pl = vals[rng.integers(0, vals.size, size=(n, G))]
    flat = rng.uniform(size=n) < p_flat
    pl[flat] = vals[rng.integers(0, vals.size, size=int(flat.sum()))][:, None]
    bad = np.nonzero(rng.uniform(size=n) < p_bad)[0]
    for i in bad:
        kind = rng.integers(0, 3)
        if kind == 0:      # a wholly missing sample
            pl[i, :] = MISSING[dtype]
        elif kind == 1:    # a haploid-style short vector: the tail is end-of-vector
            pl[i, rng.integers(1, G):] = END_OF_VECTOR[dtype]
        else:              # one missing value
            pl[i, rng.integers(0, G)] = MISSING[dtype]
    return pl.astype(dtype)


def same_bits(a, b) -> bool:
    """float32 rows equal bit for bit where they are numbers, NaN at the same positions"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))
