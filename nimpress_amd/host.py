"""ctypes binding of the C++ host layer (libnimpress_host.so): the reference's
computePolygenicScores over real files (.scores + VCF/vcf.gz [+ BED]), with the row loop on the GPU.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Tuple

import numpy as np

from . import capi

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libnimpress_host.so")
_lib = None


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise capi.NpsError(-2, "libnimpress_host.so not built (%s)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.nh_last_error.restype = C.c_char_p
        L.nh_compute.restype = C.c_long
        L.nh_compute.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int,
                                 C.c_double, C.c_double, C.c_long, C.c_int, C.c_int, C.c_void_p,
                                 C.c_long, C.POINTER(C.c_ulonglong), C.c_char_p, C.c_long]
        L.nh_compute_multi.restype = C.c_long
        L.nh_compute_multi.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_double,
                                       C.c_double, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_void_p,
                                       C.c_char_p, C.c_long]
        L.nh_compute_multi_partial.restype = C.c_long
        L.nh_compute_multi_partial.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_double,
                                               C.c_double, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                               C.c_long, C.c_void_p, C.c_void_p, C.c_char_p, C.c_long]
        L.nh_compute_dev.restype = C.c_long
        L.nh_compute_dev.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                     C.c_long, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_ulonglong), C.c_char_p, C.c_long]
        L.nh_compute_multi_dev.restype = C.c_long
        L.nh_compute_multi_dev.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_double,
                                           C.c_double, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_char_p, C.c_long]
        L.nh_compute_multi_ex.restype = C.c_long
        L.nh_compute_multi_ex.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_double,
                                          C.c_double, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint,
                                          C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_long]
        L.nh_decode_gt_dosage.restype = C.c_long
        L.nh_decode_gt_dosage.argtypes = [C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_int, C.c_void_p]
        L.nh_decode_code_dosage.restype = C.c_long
        L.nh_decode_code_dosage.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_void_p]
        L.nh_decode_pl_dosage.restype = C.c_long
        L.nh_decode_pl_dosage.argtypes = [C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_int, C.c_void_p]
        L.nh_vcf_find_pl.restype = C.c_long
        L.nh_vcf_find_pl.argtypes = [C.c_void_p, C.c_char_p, C.c_long, C.c_char_p, C.c_char_p, C.c_void_p, C.c_long]
        L.nh_last_log_size.restype = C.c_long
        L.nh_last_log.restype = C.c_long
        L.nh_last_log.argtypes = [C.c_char_p, C.c_long]
        L.nh_last_timings.restype = None
        L.nh_last_timings.argtypes = [C.c_void_p]
        L.nh_vcf_open.restype = C.c_void_p
        L.nh_vcf_open.argtypes = [C.c_char_p, C.c_char_p]
        L.nh_vcf_close.argtypes = [C.c_void_p]
        L.nh_vcf_n_samples.restype = C.c_long
        L.nh_vcf_n_samples.argtypes = [C.c_void_p]
        L.nh_vcf_open_header.restype = C.c_void_p
        L.nh_vcf_open_header.argtypes = [C.c_char_p]
        L.nh_vcf_sample.restype = C.c_char_p
        L.nh_vcf_sample.argtypes = [C.c_void_p, C.c_long]
        L.nh_vcf_samples_joined.restype = C.c_long
        L.nh_vcf_samples_joined.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
        L.nh_format_float.restype = None
        L.nh_format_float.argtypes = [C.c_double, C.c_char_p, C.c_long]
        L.nh_write_matrix_tsv.restype = C.c_long
        L.nh_write_matrix_tsv.argtypes = [C.c_char_p, C.c_char_p, C.c_long, C.c_void_p, C.c_long, C.c_long]
        _lib = L
    return _lib


def _full_log(L, buf) -> str:
    """the log text of the call that just returned: the caller's buffer, or -- when that was too small and ends in the
    library's "... log truncated" line -- the complete text the library kept (nh_last_log)"""
    size = L.nh_last_log_size()
    if size < len(buf):
        return buf.value.decode("utf-8", "replace")
    big = C.create_string_buffer(size + 1)
    L.nh_last_log(big, len(big))
    return big.value.decode("utf-8", "replace")


MULTI_ACCEPT_DS = 1   # flags of nh_compute_multi_ex: FORMAT/DS records are scored too (dosage rows, two reads)


def decode_gt_dosage(gt: np.ndarray, ploidy: int, eaidx: int) -> np.ndarray:
    """the host's decode of a typed FORMAT/GT vector (int8 / int16 / int32, n x ploidy values) into the float32 row of
    effect allele counts that the one-pass dosage route uploads (NaN = a missing allele)"""
    gt = np.ascontiguousarray(gt)
    if gt.dtype not in (np.int8, np.int16, np.int32) or gt.size % ploidy:
        raise ValueError("gt must be int8 / int16 / int32 with n * ploidy values")
    out = np.empty(max(gt.size // ploidy, 1), dtype=np.float32)
    n = load().nh_decode_gt_dosage(gt.ctypes.data, gt.dtype.itemsize, gt.size // ploidy, int(ploidy), int(eaidx), out.ctypes.data)
    if n < 0:
        raise capi.NpsError(-1, "nh_decode_gt_dosage: bad arguments")
    return out[:n]


def decode_code_dosage(codes: np.ndarray, n: int, code_map: int) -> np.ndarray:
    """the same for the ceil(n / 4) bytes of a .bed / .pgen record under its code map (NPS_MAP_*: 0 / 1 .bed A2 / A1,
    2 / 3 .pgen ALT / REF)"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    if codes.size < (n + 3) // 4:
        raise ValueError("codes too short")
    out = np.empty(max(n, 1), dtype=np.float32)
    if load().nh_decode_code_dosage(codes.ctypes.data, int(n), int(code_map), out.ctypes.data) < 0:
        raise capi.NpsError(-1, "nh_decode_code_dosage: bad arguments")
    return out[:n]


def decode_pl_dosage(pl: np.ndarray, n_alleles: int, eaidx: int) -> np.ndarray:
    """the host's decode of a typed FORMAT/PL vector (int8 / int16 / int32, n x A (A + 1) / 2 values of n diploid samples at
    a record of A = n_alleles alleles) into the float32 row of the effect allele's expected count -- the mirror of the
    device decode of nps_push_pl (include/nps.h): NaN = a missing or uninformative sample"""
    pl = np.ascontiguousarray(pl)
    G = n_alleles * (n_alleles + 1) // 2
    if pl.dtype not in (np.int8, np.int16, np.int32) or G < 1 or pl.size % G:
        raise ValueError("pl must be int8 / int16 / int32 with n * A (A + 1) / 2 values")
    out = np.empty(max(pl.size // G, 1), dtype=np.float32)
    n = load().nh_decode_pl_dosage(pl.ctypes.data, pl.dtype.itemsize, pl.size // G, int(n_alleles), int(eaidx), out.ctypes.data)
    if n < 0:
        raise capi.NpsError(-1, "nh_decode_pl_dosage: bad arguments")
    return out[:n]


class GenotypeFile:
    """a genotype file opened by the host's reader (nh_vcf_open), records kept -- for looking at what the score loop would
    see of a record.  score_path: keep only the records of that score file's loci."""

    def __init__(self, path: str, score_path: Optional[str] = None):
        self._h = load().nh_vcf_open(path.encode(), score_path.encode() if score_path else None)
        if not self._h:
            raise capi.NpsError(-1, "cannot open %s: %s" % (path, load().nh_last_error().decode("utf-8", "replace")))
        self.n_samples = int(load().nh_vcf_n_samples(self._h))

    def find_pl(self, contig: str, pos: int, ref: str, ea: str) -> Optional[np.ndarray]:
        """the FORMAT/PL dosage row of the record a score row selects (nh_vcf_find_pl): float32[n_samples]; None when the
        record found is not scored from PL (NIMPRESS_FORMAT=PL not set when the file was opened, no PL, more than 8
        alleles); KeyError when no record matches"""
        out = np.empty(max(self.n_samples, 1), dtype=np.float32)
        n = load().nh_vcf_find_pl(self._h, contig.encode(), int(pos), ref.encode(), ea.encode(), out.ctypes.data, self.n_samples)
        if n == -1:
            raise KeyError("%s:%d:%s:%s" % (contig, pos, ref, ea))
        if n < 0:
            raise capi.NpsError(-1, load().nh_last_error().decode("utf-8", "replace"))
        if n == 0 and self.n_samples:
            return None
        return out[:n]

    def close(self):
        if self._h:
            load().nh_vcf_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


TIMING_KEYS = ("hip_init_s", "hip_init_wait_s", "open_s", "inflate_parse_s", "push_s", "kernel_s", "warnings_s")


def last_timings() -> dict:
    """where the last compute_polygenic_scores* call of this thread spent its time (seconds; hip_init_s ran on a thread
    of its own beside open + inflate + parse, hip_init_wait_s is what of it the run had to wait for)"""
    t = np.zeros(7, dtype=np.float64)
    load().nh_last_timings(t.ctypes.data)
    return dict(zip(TIMING_KEYS, (float(x) for x in t)))


def compute_polygenic_scores(score_path: str, vcf_path: str, cov: Optional[str] = None,
                             imp_locus: str = "ps", imp_missing: str = "homref",
                             imp_sample: str = "int_ps", maxmis: float = 0.05, mincs: int = 100,
                             afmisp: float = 0.001, ignorefilt: bool = False, device: int = 0,
                             max_samples: int = 1 << 22, d_out: Optional[int] = None) -> Tuple[np.ndarray, int, List[str]]:
    """nimpress's main() minus the printing (CLI defaults).  Returns (scores, nloci, log lines).  d_out: a device
    pointer to n_samples doubles -- the scores are left there (nps_finish_device) and None is returned for them."""
    L = load()
    nloci = C.c_ulonglong(0)
    log = C.create_string_buffer(1 << 20)
    args = (score_path.encode(), vcf_path.encode(), cov.encode() if cov else None,
            capi.LOCUS[imp_locus], capi.MISSING[imp_missing], capi.SAMPLE[imp_sample],
            float(maxmis), float(afmisp), int(mincs), int(ignorefilt), device)
    if d_out is not None:
        scores = None
        n = L.nh_compute_dev(*args, C.c_void_p(int(d_out)), C.byref(nloci), log, len(log))
    else:
        scores = np.empty(max_samples, dtype=np.float64)
        n = L.nh_compute(*args, scores.ctypes.data, max_samples, C.byref(nloci), log, len(log))
    if n < 0:
        raise capi.NpsError(-3 if n == -2 else -1, L.nh_last_error().decode("utf-8", "replace"))
    return (None if scores is None else scores[:n].copy()), int(nloci.value), [l for l in _full_log(L, log).split("\n") if l]


def compute_polygenic_scores_multi(score_paths, vcf_path: str, cov: Optional[str] = None, imp_locus: str = "ps",
                                   imp_missing: str = "homref", imp_sample: str = "int_ps", maxmis: float = 0.05,
                                   mincs: int = 100, afmisp: float = 0.001, ignorefilt: bool = False, device: int = 0,
                                   max_samples: int = 1 << 22, d_out: Optional[int] = None, accept_ds: bool = False):
    """Several score files on one genotype file in ONE pass over the genotypes (computePolygenicScoresMulti: the union
    of the files' loci decoded once into a resident cohort, all definitions applied together on the matrix cores).
    Returns (scores [files, samples], nloci [files], log lines per file).  d_out: a device pointer to
    [files, samples] doubles (samples = the cohort's) -- the scores are left there (nps_multi_finish_device) and None is
    returned for them.  accept_ds: FORMAT/DS records are scored too -- a float32 dosage cohort, two reads for all files --
    instead of being an error."""
    L = load()
    S = len(score_paths)
    nloci = np.zeros(S, dtype=np.uint64)
    log = C.create_string_buffer(4 << 20)
    args = ("\n".join(score_paths).encode(), vcf_path.encode(), cov.encode() if cov else None,
            capi.LOCUS[imp_locus], capi.MISSING[imp_missing], capi.SAMPLE[imp_sample], float(maxmis),
            float(afmisp), int(mincs), int(ignorefilt), device)
    if accept_ds:
        scores = None if d_out is not None else np.empty((S, max_samples), dtype=np.float64)
        n = L.nh_compute_multi_ex(*args, 0, 1, 0, MULTI_ACCEPT_DS, None if scores is None else scores.ctypes.data, max_samples,
                                  None if d_out is None else C.c_void_p(int(d_out)), nloci.ctypes.data, None, log, len(log))
    elif d_out is not None:
        scores = None
        n = L.nh_compute_multi_dev(*args, 0, 1, 0, C.c_void_p(int(d_out)), nloci.ctypes.data, None, log, len(log))
    else:
        scores = np.empty((S, max_samples), dtype=np.float64)
        n = L.nh_compute_multi(*args, scores.ctypes.data, max_samples, nloci.ctypes.data, log, len(log))
    if n < 0:
        raise capi.NpsError(-3 if n == -2 else -1, L.nh_last_error().decode("utf-8", "replace"))
    return (None if scores is None else scores[:, :n].copy()), nloci.astype(np.int64), _split_logs(_full_log(L, log), S)


def _split_logs(text: str, S: int):
    """"<file index> TAB line" -> the lines of every file (a line without a valid index -- there is none unless the
    text was cut -- is dropped rather than attached to the wrong file)"""
    logs = [[] for _ in range(S)]
    for l in text.split("\n"):
        k, tab, rest = l.partition("\t")
        if tab and k.isdigit() and int(k) < S:
            logs[int(k)].append(rest)
    return logs


def compute_polygenic_scores_multi_partial(score_paths, vcf_path: str, shard: int, n_shards: int, cov: Optional[str] = None,
                                           imp_locus: str = "ps", imp_missing: str = "homref",
                                           imp_sample: str = "int_ps", maxmis: float = 0.05, mincs: int = 100,
                                           afmisp: float = 0.001, ignorefilt: bool = False, device: int = 0,
                                           max_samples: int = 1 << 22, d_out: Optional[int] = None,
                                           accept_ds: bool = False):
    """Rows sharded over several GPUs x ALL score files on each: block `shard` of `n_shards` of
    the union of the files' loci is located, decoded and scored on this GPU -- 1 / n_shards of the ingest and of the
    cohort.  Returns (sums [files, samples] BEFORE the normalisation, nloci [files] of the block, offsets [files],
    log lines per file for the block's rows); the caller sum-all-reduces sums and nloci over the shards
    (multi.all_reduce_partial_matrix) and applies sums / (2 nloci) + offset (multi.normalize_matrix)."""
    L = load()
    S = len(score_paths)
    nloci = np.zeros(S, dtype=np.uint64)
    offsets = np.zeros(S, dtype=np.float64)
    log = C.create_string_buffer(4 << 20)
    args = ("\n".join(score_paths).encode(), vcf_path.encode(), cov.encode() if cov else None,
            capi.LOCUS[imp_locus], capi.MISSING[imp_missing], capi.SAMPLE[imp_sample],
            float(maxmis), float(afmisp), int(mincs), int(ignorefilt), device, int(shard), int(n_shards))
    if accept_ds:           # (FORMAT/DS records are scored too: compute_polygenic_scores_multi)
        sums = None if d_out is not None else np.zeros((S, max_samples), dtype=np.float64)
        n = L.nh_compute_multi_ex(*args, 1, MULTI_ACCEPT_DS, None if sums is None else sums.ctypes.data, max_samples,
                                  None if d_out is None else C.c_void_p(int(d_out)), nloci.ctypes.data, offsets.ctypes.data,
                                  log, len(log))
    elif d_out is not None:   # the block's sums stay on the device for the all-reduce (nps_multi_partial_device)
        sums = None
        n = L.nh_compute_multi_dev(*args, 1, C.c_void_p(int(d_out)), nloci.ctypes.data, offsets.ctypes.data, log, len(log))
    else:
        sums = np.zeros((S, max_samples), dtype=np.float64)
        n = L.nh_compute_multi_partial(*args, sums.ctypes.data, max_samples, nloci.ctypes.data, offsets.ctypes.data,
                                       log, len(log))
    if n < 0:
        raise capi.NpsError(-3 if n == -2 else -1, L.nh_last_error().decode("utf-8", "replace"))
    return (None if sums is None else sums[:, :n].copy()), nloci.astype(np.int64), offsets, _split_logs(_full_log(L, log), S)


def format_scores(x: np.ndarray) -> List[str]:
    """format_score over an array, without a C call per value: "%.16g" with ".0" appended where the text has no
    '.', 'e', 'n' or 'i' (nimpress.nim:753; pinned by scores/*_nimpress_res.txt)"""
    out = np.char.mod("%.16g", np.asarray(x, dtype=np.float64))
    plain = ~(np.char.find(out, ".") >= 0) & ~(np.char.find(out, "e") >= 0) & ~(np.char.find(out, "n") >= 0) & \
        ~(np.char.find(out, "i") >= 0)
    return np.where(plain, np.char.add(out, ".0"), out).tolist()


def write_matrix_tsv(path: str, names: List[str], scores: np.ndarray) -> None:
    """scores [n_scores, n_samples] -> one line per sample, `name TAB score 1 TAB score 2 ...`, every value in the
    reference's float format (nimpress.nim:752-753); formatted by up to 16 threads of the host library
    (nh_write_matrix_tsv).  path "-" writes to stdout."""
    m = np.ascontiguousarray(scores, dtype=np.float64)
    if m.ndim != 2 or m.shape[1] != len(names):
        raise ValueError("scores must be [n_scores, %d]" % len(names))
    if any("\n" in s for s in names):
        raise ValueError("a sample name contains a newline")
    if path == "-":
        import sys
        sys.stdout.flush()
    rc = load().nh_write_matrix_tsv(path.encode(), "\n".join(names).encode(), len(names), m.ctypes.data, m.shape[0],
                                    m.shape[1])
    if rc != 0:
        raise capi.NpsError(-1, load().nh_last_error().decode("utf-8", "replace"))


def sample_names(vcf_path: str) -> List[str]:
    """samples(vcf) of the reference (nimpress.nim:753): the header's sample names, in order"""
    L = load()
    h = L.nh_vcf_open_header(vcf_path.encode())
    if not h:
        raise capi.NpsError(-1, "cannot open %s: %s" % (vcf_path, L.nh_last_error().decode("utf-8", "replace")))
    try:
        if L.nh_vcf_n_samples(h) == 0:
            return []
        need = L.nh_vcf_samples_joined(h, None, 0)
        buf = C.create_string_buffer(need + 1)
        L.nh_vcf_samples_joined(h, buf, need + 1)
        return buf.raw[:need].decode().split("\n")
    finally:
        L.nh_vcf_close(h)


def format_score(x: float) -> str:
    """Nim's `$float` as the reference prints it (nimpress.nim:753; "%.16g", ".0" for integers, "nan")"""
    buf = C.create_string_buffer(64)
    load().nh_format_float(float(x), buf, len(buf))
    return buf.value.decode()
