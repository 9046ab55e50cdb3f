"""The file-driven one-pass path over FORMAT/DS files (computePolygenicScoresMulti with acceptDs, score_many.py
--ds-one-pass): three score files over one genotype file, scored together from a float32 dosage cohort in two reads,
against the same files scored one by one (computePolygenicScores: nps_push_ds / nps_push_gt per row).  Scores within
test_gpu_multi's bar, nloci identical, the sorted WARN lines identical at the default --afmisp.  Without the option
nothing changes: tests/test_gpu_scorefiles.py pins that."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from nimpress_amd import capi, host
from test_gpu_cli import _ds_cohort, _write_ds_files
from test_gpu_multi import REL_TOL, rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, M = 3000, 40


def write_score_files(tmp_path, entries):
    """three definitions over the same loci: the cohort's own betas, then two other sets (one drops every fourth locus)"""
    rng = np.random.default_rng(5)
    paths, betas = [], []
    for s in range(3):
        beta = [e.beta if s == 0 else float(np.round(rng.normal(0, 0.05 * (1 + s)), 4)) for e in entries]
        keep = [j for j in range(len(entries)) if not (s == 2 and j % 4 == 1)]
        p = str(tmp_path / ("def%d.score" % s))
        with open(p, "w") as f:
            f.write("ds test %d\n\n\nGRCh37\n%r\n" % (s, 0.25 * s))
            f.write("\n".join("%s\t%d\t%s\t%s\t%r\t%s" % (entries[j].contig, entries[j].pos, entries[j].refseq, entries[j].easeq,
                                                         beta[j], "NaN" if np.isnan(entries[j].eaf) else repr(entries[j].eaf))
                              for j in keep))
        paths.append(p)
        betas.append([abs(beta[j]) for j in keep])
    return paths, betas


def write_mixed_vcf(tmp_path, samples, recs):
    """a text VCF whose records carry GT and DS (scored from GT), DS alone, or GT alone, in turn"""
    path = str(tmp_path / "mixed.vcf.gz")
    with gzip.open(path, "wt") as f:
        f.write("##fileformat=VCFv4.2\n##contig=<ID=7>\n"
                '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n'
                '##FORMAT=<ID=DS,Number=A,Type=Float,Description="ALT allele dosage">\n')
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(samples) + "\n")
        for k, r in enumerate(recs):
            d = r.ds[:, 0]
            ds = ["." if np.isnan(x) else ("%.3f" % x).rstrip("0").rstrip(".") for x in d]
            gt = ["./." if np.isnan(x) else ("0/0", "0/1", "1/1")[int(np.clip(np.rint(x), 0, 2))] for x in d]
            fmt, vals = (("GT:DS", [a + ":" + b for a, b in zip(gt, ds)]), ("DS", ds), ("GT", gt))[k % 3]
            f.write("%s\t%d\t.\t%s\t%s\t.\t%s\t.\t%s\t%s\n" % (r.contig, r.pos, r.ref, ",".join(r.alts), r.filt, fmt, "\t".join(vals)))
    return path


def warn_lines(log):
    return sorted(l for l in log if l.startswith("WARN"))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("multi_ds")
    entries, recs = _ds_cohort(N, M, 4242)
    _, bcf, samples = _write_ds_files(tmp, N, entries, recs, text=False)
    mixed = write_mixed_vcf(tmp, samples, recs)
    paths, betas = write_score_files(tmp, entries)
    return dict(tmp=tmp, bcf=bcf, mixed=mixed, scores=paths, betas=betas, samples=samples)


@pytest.mark.parametrize("which", ["bcf", "mixed"])
@pytest.mark.parametrize("kw", [dict(), dict(imp_locus="homref", imp_sample="int_fail", maxmis=0.08, mincs=10)])
def test_accept_ds_equals_file_by_file(files, which, kw):
    cohort = files[which]
    with pytest.raises(capi.NpsError) as e:           # the default has not moved
        host.compute_polygenic_scores_multi(files["scores"], cohort, **kw)
    assert "one-pass" in str(e.value)
    got, nloci, logs = host.compute_polygenic_scores_multi(files["scores"], cohort, accept_ds=True, **kw)
    assert got.shape == (3, N)
    warned = 0
    for s, path in enumerate(files["scores"]):
        ref, ref_nloci, ref_log = host.compute_polygenic_scores(path, cohort, **kw)
        assert int(nloci[s]) == ref_nloci
        assert rel_err(got[s], ref, float(np.sum(files["betas"][s])), ref_nloci) <= REL_TOL, (which, s)
        assert warn_lines(logs[s]) == warn_lines(ref_log), (which, s)
        warned += len(warn_lines(ref_log))
    assert warned > 0


def test_score_many_ds_one_pass(files):
    tmp = files["tmp"]
    tool = os.path.join(ROOT, "tools", "score_many.py")

    def run(out, *flags):
        r = subprocess.run([sys.executable, tool, "--gpus", "1", *flags, "--out", str(tmp / out), *files["scores"], files["bcf"]],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        rows = [l.split("\t") for l in open(tmp / out).read().splitlines()]
        assert [x[0] for x in rows] == files["samples"]
        return np.array([[float(v) for v in x[1:]] for x in rows]).T, r.stderr

    one, err = run("one.tsv", "--ds-one-pass")
    assert "(one pass over the genotypes, dosage rows)" in err
    ref, err_ref = run("ref.tsv")
    assert "one pass" not in err_ref
    assert one.shape == ref.shape == (3, N)
    for s in range(3):
        assert rel_err(one[s], ref[s], float(np.sum(files["betas"][s])), M) <= REL_TOL, s
    assert sorted(l for l in err.splitlines() if "WARN" in l) == sorted(l for l in err_ref.splitlines() if "WARN" in l)


def test_accept_ds_row_shards_add_up(files):
    """the rows-sharded layout (compute_polygenic_scores_multi_partial) with accept_ds: the un-normalised sums and the
    locus counts of two blocks of the union's rows add up to the one-call result"""
    whole, nloci, _ = host.compute_polygenic_scores_multi(files["scores"], files["mixed"], accept_ds=True)
    sums, total, offs = np.zeros((3, N)), np.zeros(3, np.int64), None
    for shard in range(2):
        with pytest.raises(capi.NpsError):             # the default has not moved here either
            host.compute_polygenic_scores_multi_partial(files["scores"], files["bcf"], shard, 2)
        s, nl, offs, _ = host.compute_polygenic_scores_multi_partial(files["scores"], files["mixed"], shard, 2, accept_ds=True)
        sums += s
        total += nl
    assert np.array_equal(total, nloci)
    got = sums / (2.0 * total)[:, None] + offs[:, None]
    for s in range(3):
        assert rel_err(got[s], whole[s], float(np.sum(files["betas"][s])), int(total[s])) <= REL_TOL, s
