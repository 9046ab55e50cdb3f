"""FORMAT/PL end to end: the `nimpress` command line with NIMPRESS_FORMAT=PL on a 2 000-sample indexed BCF (int16 PL; the
streaming-window path) and on a 500-sample text vcf.gz, against a Python restatement -- the records tests/plfiles.py wrote
-> pl_reference.pl_dosage -> the oracle's row_ds / row_gt per record -> format_score.

The ALT-effect score file is an exact design (tests/exact_reference.py): PL values of at most 30 keep every dosage above
2^-13 (a float32 multiple of 2^-36), betas are multiples of 2^-6 below 1 and eafs multiples of 2^-4 under --imp-sample=ps, so
every term and every partial sum of the at most 40 rows is a multiple of 2^-42 below 2^7: an exact double in ANY order of
summation.  The output text must then equal the restatement's byte for byte, and one wrong bit in one dosage shows.  The
REF-effect score file runs under the defaults (int_ps) and is held to the float64 bound of exact_reference.f64_bound."""
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_reference as er
import pl_reference as plr
import plfiles
from nimpress_amd import capi
from oracle import refcpu
from test_gpu_multi import REL_TOL, rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "nimpress_amd", "nimpress")
M = 36
PL_VALUES = np.array([3, 10, 20, 30])


def make_records(n, seed):
    """M loci on two contigs.  j % 6 == 4: GT only; j == 13: 9 alleles (GT is used); j % 11 == 7: FILTER FAIL; j % 3 == 1:
    three alleles; per-record share of uninformative samples ('.', a flat vector or a short one) 0 .. 12 %"""
    rng = np.random.default_rng(seed)
    recs = []
    for j in range(M):
        n_alt = 8 if j == 13 else (2 if j % 3 == 1 else 1)
        A = n_alt + 1
        eaf = float(rng.integers(1, 8)) / 16.0
        a = (rng.uniform(size=(n, 2)) < eaf).astype(np.int64) * rng.integers(1, n_alt + 1, size=(n, 2))
        a.sort(axis=1)
        gts = (a + 1) << 1
        gts[rng.uniform(size=n) < 0.02] = 0
        pl = None
        if j % 6 != 4:
            G = plr.n_genotypes(A)
            pl = PL_VALUES[rng.integers(0, PL_VALUES.size, size=(n, G))]
            pl[np.arange(n), a[:, 1] * (a[:, 1] + 1) // 2 + a[:, 0]] = 0       # the called genotype is the likeliest
            bad = np.nonzero(rng.uniform(size=n) < 0.12 * (j % 5) / 4.0)[0]
            for i in bad:
                k = rng.integers(0, 3)
                pl[i] = plfiles.PL_MISSING if k == 0 else (0 if k == 1 else pl[i])
                if k == 2:
                    pl[i, G - 1:] = plfiles.PL_EOV
        recs.append(dict(contig="7" if j < M // 2 else "9", pos=1000 + 53 * j, ref="A",
                         alts=["G", "T", "C", "AA", "AC", "AG", "AT", "CA"][:n_alt],
                         filters=["FAIL"] if j % 11 == 7 else (["PASS"] if j % 2 else []), gts=gts, pl=pl, eaf=eaf))
    return recs


def score_rows(recs, effect_ref, seed):
    """one score row per record (+ two absent loci); effect_ref: every other PL record counts REF"""
    rng = np.random.default_rng(seed)
    rows = []
    for j, r in enumerate(recs):
        ea = r["ref"] if (effect_ref and j % 2 == 0) else r["alts"][-1]
        rows.append((r["contig"], r["pos"], r["ref"], ea, float(rng.integers(-40, 41)) / 64.0, r["eaf"]))
        if j % 17 == 5:
            rows.append((r["contig"], r["pos"] + 7, "C", "T", 0.25, 0.125))        # absent
    return rows


def restate(recs, rows, n, dtype, table, use_pl):
    """per score row what the loop does with it: ('locus', kind) / ('ds', float32 row, counts effect) / ('gt', int32 gts, eaidx)"""
    by_locus = {(r["contig"], r["pos"]): r for r in recs}
    out = []
    for c, p, ref, ea, beta, eaf in rows:
        r = by_locus.get((c, p))
        if r is None or r["ref"] != ref:
            out.append(("locus", capi.ROW_ABSENT))
        elif r["filters"] not in ([], ["PASS"]):
            out.append(("locus", capi.ROW_FILTERED))
        else:
            A = 1 + len(r["alts"])
            e = 0 if ea == ref else r["alts"].index(ea) + 1
            if use_pl and r["pl"] is not None and A <= 8:
                out.append(("ds", plr.pl_dosage(plfiles.typed_pl(r["pl"], dtype), A, e, table), e))
            else:
                out.append(("gt", r["gts"].astype(np.int32), e))
    return out


def oracle_text(samples, rows, plan, n, kw, offset):
    sc = refcpu.RefScorer(n, refcpu.make_params(**kw))
    for (c, p, ref, ea, beta, eaf), step in zip(rows, plan):
        rie = ref == ea
        if step[0] == "locus":
            sc.row_locus(step[1], rie, beta, eaf)
        elif step[0] == "ds":
            assert not rie                     # (the oracle's row_ds would take 2 - DS: ALT-effect rows only)
            sc.row_ds(step[1], False, beta, eaf)
        else:
            sc.row_gt(step[1].ravel(), 2, step[2], rie, beta, eaf)
    scores, nloci = sc.finish(offset)
    return "".join("%s\t%s\n" % (s, refcpu.format_score(x)) for s, x in zip(samples, scores)), nloci, sc.stats


def run_cli(flags, score, path, env_format, window=None):
    env = dict(os.environ)
    env.pop("NIMPRESS_FORMAT", None)
    env.pop("NIMPRESS_WINDOW", None)
    if env_format:
        env["NIMPRESS_FORMAT"] = env_format
    if window:
        env["NIMPRESS_WINDOW"] = str(window)
    r = subprocess.run([CLI, *flags, score, path], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    return "".join(l + "\n" for l in lines if not l.startswith(("WARN ", "FATAL "))), [l for l in lines if l.startswith("WARN ")]


@pytest.fixture(scope="module")
def table():
    return capi.pl_likelihoods()


@pytest.fixture(scope="module", params=["bcf", "text"])
def files(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pl_" + request.param)
    n = 2000 if request.param == "bcf" else 500
    samples = ["P%05d" % i for i in range(n)]
    recs = make_records(n, 11 + n)
    bare = [dict(r, pl=None) for r in recs]
    if request.param == "bcf":
        path, twin, dtype = str(tmp / "pl.bcf"), str(tmp / "bare.bcf"), np.int16
        plfiles.write_bcf(path, ["7", "9"], samples, recs, pl_dtype=np.int16)
        plfiles.write_bcf(twin, ["7", "9"], samples, bare)
    else:
        path, twin, dtype = str(tmp / "pl.vcf.gz"), str(tmp / "bare.vcf.gz"), np.int32
        plfiles.write_vcf(path, samples, recs)
        plfiles.write_vcf(twin, samples, bare)
    alt_rows, ref_rows = score_rows(recs, False, 3), score_rows(recs, True, 4)
    alt_score, ref_score = str(tmp / "alt.score"), str(tmp / "ref.score")
    plfiles.write_score(alt_score, alt_rows, offset=0.25)
    plfiles.write_score(ref_score, ref_rows, offset=0.0)
    return dict(kind=request.param, n=n, samples=samples, recs=recs, path=path, twin=twin, dtype=dtype, tmp=tmp,
                alt_rows=alt_rows, ref_rows=ref_rows, alt_score=alt_score, ref_score=ref_score)


EXACT_FLAGS = ["--imp-sample=ps", "--afmisp=0"]
EXACT_KW = dict(imp_locus="ps", imp_missing="homref", imp_sample="ps", maxmis=0.05, mincs=100)


def test_cli_alt_effect_rows_equal_the_restatement_text(files, table):
    f = files
    plan = restate(f["recs"], f["alt_rows"], f["n"], f["dtype"], table, use_pl=True)
    assert sum(s[0] == "ds" for s in plan) >= 20 and sum(s[0] == "gt" for s in plan) >= 5 and sum(s[0] == "locus" for s in plan) >= 4
    want, nloci, stats = oracle_text(f["samples"], f["alt_rows"], plan, f["n"], EXACT_KW, 0.25)
    over = [s[4] == capi.REASON_MAXMIS for s, step in zip(stats, plan) if step[0] == "ds"]
    assert 0 < sum(over) < len(over)                       # PL rows on both sides of --maxmis
    got, warns = run_cli(EXACT_FLAGS, f["alt_score"], f["path"], "PL", window=7 if f["kind"] == "bcf" else None)
    assert got == want
    assert sum("missingness threshold" in w for w in warns) == sum(s[4] == capi.REASON_MAXMIS for s in stats)
    if f["kind"] == "bcf":   # lower case is accepted too, and one window instead of six changes nothing
        assert run_cli(EXACT_FLAGS, f["alt_score"], f["path"], "pl")[0] == want


def test_cli_without_the_variable_scores_gt_as_today(files, table):
    """unset and DS: the PL file gives exactly the output of its twin that carries no PL at all, which is the oracle's
    GT-scored output"""
    f = files
    plan = restate(f["recs"], f["alt_rows"], f["n"], f["dtype"], table, use_pl=False)
    want, _, _ = oracle_text(f["samples"], f["alt_rows"], plan, f["n"], EXACT_KW, 0.25)
    twin = run_cli(EXACT_FLAGS, f["alt_score"], f["twin"], None)
    assert twin[0] == want
    for env in (None, "DS"):
        assert run_cli(EXACT_FLAGS, f["alt_score"], f["path"], env) == twin
    if f["kind"] == "text":
        assert run_cli(EXACT_FLAGS, f["alt_score"], f["twin"], "PL") == twin     # nothing to select: GT


def test_cli_ref_effect_rows_within_f64_bound(files, table):
    """defaults (int_ps): half of the PL rows count REF.  The row holds the REF count itself (e = 0), ref_is_effect only
    selects the homref value: the double-double reference on the numpy dosages with rie = 1, within f64_bound plus the
    u |score| of reading a score back from its 16 printed digits"""
    f = files
    kw = dict(imp_locus="ps", imp_missing="homref", imp_sample="int_ps", maxmis=0.05, mincs=100)
    plan = restate(f["recs"], f["ref_rows"], f["n"], f["dtype"], table, use_pl=True)
    dos, kind = [], []
    for step in plan:
        kind.append(step[1] if step[0] == "locus" else 0)
        if step[0] == "ds":
            dos.append(step[1].astype(np.float64))
        elif step[0] == "gt":
            g = step[1]
            cnt = (((g >> 1) - 1) == step[2]).sum(axis=1).astype(np.float64)
            cnt[(g < 2).any(axis=1)] = np.nan
            dos.append(cnt)
    beta = np.array([r[4] for r in f["ref_rows"]])
    eaf = np.array([r[5] for r in f["ref_rows"]])
    rie = np.array([int(r[2] == r[3]) for r in f["ref_rows"]], np.int32)
    assert sum(1 for s, r in zip(plan, rie) if s[0] == "ds" and r) >= 10
    hi, lo, ab, nl, _, _, _ = er.dd_reference(np.array(dos), beta, eaf, rie, kw, np.array(kind, np.int32))
    text, _ = run_cli(["--afmisp=0"], f["ref_score"], f["path"], "PL", window=5 if f["kind"] == "bcf" else None)
    rows = [l.split("\t") for l in text.splitlines()]
    assert [x[0] for x in rows] == f["samples"]
    got = np.array([float(x[1]) for x in rows])
    ok = np.isfinite(got)
    assert ok.all() and np.isfinite(hi).all()
    bound = er.f64_bound(ab, nl, got, nl) + er.U * np.abs(got) * 2 * nl
    assert np.all(er.sum_error(got, nl, hi, lo) <= bound)


def test_score_many_ds_one_pass_over_pl(files):
    """two score files over the PL BCF in one pass (dosage rows decoded on the host: decodePlDosage) equal the file-by-file
    runs (nps_push_pl)"""
    f = files
    if f["kind"] != "bcf":
        return
    tool = os.path.join(ROOT, "tools", "score_many.py")
    env = dict(os.environ, NIMPRESS_FORMAT="PL")
    scores = [f["alt_score"], f["ref_score"]]

    def run(out, *flags):
        r = subprocess.run([sys.executable, tool, "--gpus", "1", *flags, "--out", str(f["tmp"] / out), *scores, f["path"]],
                           capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        rows = [l.split("\t") for l in open(f["tmp"] / out).read().splitlines()]
        assert [x[0] for x in rows] == f["samples"]
        return np.array([[float(v) for v in x[1:]] for x in rows]).T, r.stderr

    one, err = run("one.tsv", "--ds-one-pass")
    assert "(one pass over the genotypes, dosage rows)" in err
    ref, err_ref = run("ref.tsv")
    assert "one pass" not in err_ref
    assert one.shape == ref.shape == (2, f["n"])
    for s, rows in enumerate((f["alt_rows"], f["ref_rows"])):
        assert rel_err(one[s], ref[s], float(sum(abs(r[4]) for r in rows)), len(rows)) <= REL_TOL, s
    assert sorted(l for l in err.splitlines() if "WARN" in l) == sorted(l for l in err_ref.splitlines() if "WARN" in l)
