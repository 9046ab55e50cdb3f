"""CPU tests of FORMAT/PL on the host: the host mirror of the device decode (decodePlDosage) against the numpy restatement
of include/nps.h bit for bit, the text and BCF readers under NIMPRESS_FORMAT=PL (and unchanged behaviour without it), and
the readers alone under AddressSanitizer + UBSan on malformed PL fields (a stand-alone program, tests/native/pl_driver.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import bcfwriter
import plfiles
import pl_reference as plr
from nimpress_amd import capi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (np.int8, np.int16, np.int32)


@pytest.fixture(scope="module")
def table():
    return capi.pl_likelihoods()


# ------------------------------------------------------------------------------------------------------------------
# the decode
def test_host_decode_equals_reference_bit_for_bit(table):
    rng = np.random.default_rng(20261)
    n_nan = n_all = 0
    for A in (2, 3, 4, 8):
        for dtype in WIDTHS:
            for n in (1, 255, 256, 257, 1031):
                pl = plr.random_pl(rng, n, A, dtype)
                for e in range(A):
                    ref = plr.pl_dosage(pl, A, e, table)
                    got = host.decode_pl_dosage(pl, A, e)
                    assert got.dtype == np.float32 and plr.same_bits(got, ref), (A, dtype, n, e)
                    ok = ~np.isnan(ref)
                    assert np.all((ref[ok] >= 0) & (ref[ok] <= 2))
                    n_nan += int(np.isnan(ref).sum())
                    n_all += n
                if n >= 255:   # neither branch goes untested in any case large enough to have a share
                    share = np.isnan(plr.pl_dosage(pl, A, 0, table)).mean()
                    assert 0.05 <= share <= 0.40, (A, dtype, n, share)
    assert 0.05 <= n_nan / n_all <= 0.40


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_hand_made_rows(table, dtype):
    eov = plr.END_OF_VECTOR[np.dtype(dtype)]
    pl = np.array([[0, 0, 0], [7, 7, 7], [0, 255, 255], [0, 256, 9999], [0, 30, 300], [40, 40, eov], [30, 0, 255]], dtype=dtype)
    d1, d0 = host.decode_pl_dosage(pl, 2, 1), host.decode_pl_dosage(pl, 2, 0)
    for d in (d0, d1):
        assert np.isnan(d[0]) and np.isnan(d[1])          # flat vectors: uninformative, not dosage 1
        assert np.isnan(d[5])                             # haploid-padded sample (p, p, end of vector)
        assert d[2].view(np.uint32) == d[3].view(np.uint32)   # the cap at 255
    # 0,30,300 by hand: w = 1, 1e-3, T[255]
    w = np.array([table[0], table[30], table[255]])
    den = (w[0] + w[1]) + w[2]
    assert d1[4] == np.float32(((0.0 + 1.0 * w[1]) + 2.0 * w[2]) / den)
    assert d0[4] == np.float32(((2.0 * w[0]) + 1.0 * w[1]) / den)
    assert abs(float(d1[4]) - 1e-3 / 1.001) < 1e-9 and abs(float(d0[4]) + float(d1[4]) - 2.0) < 1e-6
    assert plr.same_bits(d1, plr.pl_dosage(pl, 2, 1, table)) and plr.same_bits(d0, plr.pl_dosage(pl, 2, 0, table))
    assert abs(float(d1[6]) - 1.0) < 2e-3                 # a confident het


def test_decode_refuses_bad_arguments():
    pl = np.zeros(3, np.int8)
    for A, e in ((1, 0), (9, 0), (2, 2), (2, -1)):
        assert host.load().nh_decode_pl_dosage(pl.ctypes.data, 1, 1, A, e, pl.ctypes.data) == -1
    assert host.load().nh_decode_pl_dosage(pl.ctypes.data, 3, 1, 2, 0, pl.ctypes.data) == -1


# ------------------------------------------------------------------------------------------------------------------
# the readers
SAMPLES = ["S%d" % i for i in range(7)]
M, E = plfiles.PL_MISSING, plfiles.PL_EOV


def gt_rows(rng, n_alt):
    a = rng.integers(0, n_alt + 1, size=(len(SAMPLES), 2))
    g = ((a + 1) << 1).astype(np.int64)
    g[rng.integers(0, len(SAMPLES))] = 0
    return g


def make_records(small: bool):
    """6 records x 7 samples; small: every PL value fits int8"""
    rng = np.random.default_rng(5)
    vals = np.array(plr.VALUES_INT8 if small else plr.VALUES_WIDE)
    alts8 = ["C", "G", "T", "AA", "AC", "AG", "AT", "CA"]                    # 9 alleles
    recs = []
    pl = vals[rng.integers(0, vals.size, size=(7, 3))]
    recs.append(dict(contig="1", pos=100, ref="A", alts=["G"], filters=[], gts=gt_rows(rng, 1), pl=pl))
    pl = vals[rng.integers(0, vals.size, size=(7, 6))]
    recs.append(dict(contig="1", pos=200, ref="A", alts=["G", "T"], filters=["PASS"], gts=gt_rows(rng, 2), pl=pl))
    recs.append(dict(contig="1", pos=300, ref="C", alts=["T"], filters=[], gts=gt_rows(rng, 1), pl=None))
    pl = vals[rng.integers(0, vals.size, size=(7, 45))]
    recs.append(dict(contig="2", pos=400, ref="A", alts=alts8, filters=[], gts=gt_rows(rng, 8), pl=pl))
    pl = vals[rng.integers(0, vals.size, size=(7, 3))]
    pl[1] = [M, M, M]           # "." in text
    pl[2] = [0, 0, 0]           # flat
    pl[3] = [5, 5, E]           # short vector
    pl[4] = [0, M, 30]          # one missing value
    recs.append(dict(contig="2", pos=500, ref="G", alts=["A"], filters=[], gts=gt_rows(rng, 1), pl=pl))
    pl = vals[rng.integers(0, vals.size, size=(7, 3))]
    recs.append(dict(contig="3", pos=600, ref="T", alts=["C"], filters=["FAIL"], gts=gt_rows(rng, 1), pl=pl))
    return recs


def score_rows(recs):
    rows = []
    for r in recs:
        rows.append((r["contig"], r["pos"], r["ref"], r["alts"][-1], 0.1, 0.2))   # an ALT is the effect allele
        rows.append((r["contig"], r["pos"], r["ref"], r["ref"], -0.2, 0.3))       # REF is
    return rows


def write_pair(tmp_path, kind):
    """the PL file of a kind and its twin without PL (the same records, GT only)"""
    small = kind == "bcf8"
    recs = make_records(small)
    bare = [dict(r, pl=None) for r in recs]
    if kind == "text":
        paths = str(tmp_path / "pl.vcf"), str(tmp_path / "bare.vcf")
        plfiles.write_vcf(paths[0], SAMPLES, recs)
        plfiles.write_vcf(paths[1], SAMPLES, bare)
        dtype = np.int32
    else:
        dtype = np.int8 if small else np.int16
        paths = str(tmp_path / "pl.bcf"), str(tmp_path / "bare.bcf")
        plfiles.write_bcf(paths[0], ["1", "2", "3"], SAMPLES, recs, pl_dtype=dtype)
        plfiles.write_bcf(paths[1], ["1", "2", "3"], SAMPLES, bare, pl_dtype=dtype)
    return recs, paths, dtype


def hooks():
    L = host.load()
    L.nh_vcf_find.restype = C.c_long
    L.nh_vcf_find.argtypes = [C.c_void_p, C.c_char_p, C.c_long, C.c_char_p, C.c_char_p, C.POINTER(C.c_long),
                              C.POINTER(C.c_int), C.c_char_p, C.c_long, C.c_void_p, C.c_long]
    L.nh_vcf_find_ds.restype = C.c_long
    L.nh_vcf_find_ds.argtypes = [C.c_void_p, C.c_char_p, C.c_long, C.c_char_p, C.c_char_p, C.c_void_p, C.c_long]
    L.nh_classify.restype = C.c_long
    L.nh_classify.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_char_p, C.c_long]
    return L


def find_all(L, gf, rows):
    """what nh_vcf_find and nh_vcf_find_ds say for every score row"""
    out = []
    for c, p, ref, ea, _, _ in rows:
        pos, ploidy = C.c_long(-1), C.c_int(-1)
        filt = C.create_string_buffer(64)
        gts = np.full(32, -77, np.int32)
        k = L.nh_vcf_find(gf._h, c.encode(), p, ref.encode(), ea.encode(), C.byref(pos), C.byref(ploidy), filt, 64,
                          gts.ctypes.data, 32)
        ds = np.zeros(8, np.float32)
        kd = L.nh_vcf_find_ds(gf._h, c.encode(), p, ref.encode(), ea.encode(), ds.ctypes.data, 8)
        out.append((k, pos.value, ploidy.value, filt.value, gts.tolist(), kd))
    return out


def classify(L, score, path):
    cap = 32
    arr = [np.zeros(cap, np.int32) for _ in range(4)]
    filt = C.create_string_buffer(1024)
    n = L.nh_classify(score.encode(), path.encode(), None, 0, cap, *[a.ctypes.data for a in arr], filt, 1024)
    assert n >= 0, L.nh_last_error()
    return n, [a[:n].tolist() for a in arr], filt.value


@pytest.mark.parametrize("kind", ["text", "bcf8", "bcf16"])
def test_reader_selects_pl_only_when_asked(tmp_path, monkeypatch, table, kind):
    L = hooks()
    recs, (with_pl, bare), dtype = write_pair(tmp_path, kind)
    rows = score_rows(recs)
    score = str(tmp_path / "t.score")
    plfiles.write_score(score, rows)

    # unset (and DS): PL is ignored -- every hook answers as for the twin file that has no PL at all
    for env in (None, "DS"):
        if env:
            monkeypatch.setenv("NIMPRESS_FORMAT", env)
        else:
            monkeypatch.delenv("NIMPRESS_FORMAT", raising=False)
        with host.GenotypeFile(with_pl) as a, host.GenotypeFile(bare) as b:
            fa, fb = find_all(L, a, rows), find_all(L, b, rows)
            assert fa == fb
            assert all(f[0] >= 0 and f[5] == 0 and f[4][:14] != [-77] * 14 for f in fa)     # GT everywhere
            for c, p, ref, ea, _, _ in rows:
                assert a.find_pl(c, p, ref, ea) is None
        assert classify(L, score, with_pl) == classify(L, score, bare)

    # NIMPRESS_FORMAT=PL: PL where present (2 .. 8 alleles), GT elsewhere
    monkeypatch.setenv("NIMPRESS_FORMAT", "PL")
    with host.GenotypeFile(with_pl) as a, host.GenotypeFile(bare) as b:
        fa, fb = find_all(L, a, rows), find_all(L, b, rows)
        for r in recs:
            A = 1 + len(r["alts"])
            for ea, e in ((r["alts"][-1], A - 1), (r["ref"], 0)):
                got = a.find_pl(r["contig"], r["pos"], r["ref"], ea)
                k = rows.index(next(x for x in rows if x[:4] == (r["contig"], r["pos"], r["ref"], ea)))
                if r["pl"] is None or A > 8:          # no PL, or the 9-allele record: its GT, as without the variable
                    assert got is None
                    assert fa[k] == fb[k] and fa[k][4][:14] != [-77] * 14
                else:
                    ref_row = plr.pl_dosage(plfiles.typed_pl(r["pl"], dtype), A, e, table)
                    assert plr.same_bits(got, ref_row), (r["pos"], ea)
                    assert fa[k][0] == fb[k][0] and fa[k][1] == r["pos"] and fa[k][4] == [-77] * 32   # the GT is not kept
                    assert fa[k][5] == 0
        special = a.find_pl("2", 500, "G", "A")
        assert np.isnan(special[1:5]).all() and not np.isnan(special[0])
        with pytest.raises(KeyError):
            a.find_pl("1", 101, "A", "G")
    # the classification of the rows does not depend on where the dosage comes from
    assert classify(L, score, with_pl) == classify(L, score, bare)


def test_reader_errors_name_the_record(tmp_path, monkeypatch):
    monkeypatch.setenv("NIMPRESS_FORMAT", "PL")
    recs = make_records(False)[:2]
    # BCF: a PL vector of 3 values at a record of 3 alleles
    bad = [dict(recs[0]), dict(recs[1], pl=recs[1]["pl"][:, :3])]
    p = str(tmp_path / "len.bcf")
    plfiles.write_bcf(p, ["1"], SAMPLES, bad)
    with pytest.raises(capi.NpsError) as e:
        host.GenotypeFile(p)
    assert all(s in str(e.value) for s in ("1:200", "3 values", "6 expected"))
    # text: a non-integer
    lines = plfiles.vcf_lines(SAMPLES, recs)
    cells = lines[-1].split("\t")
    cells[11] = cells[11].split(":")[0] + ":0,x3,7,1,2,3"
    lines[-1] = "\t".join(cells)
    p = str(tmp_path / "nonint.vcf")
    open(p, "w").write("\n".join(lines) + "\n")
    with pytest.raises(capi.NpsError) as e:
        host.GenotypeFile(p)
    assert "1:200" in str(e.value) and "x3" in str(e.value)
    # more than 8 alleles and nothing else to score from
    nine = dict(make_records(False)[3], gts=None)
    p = str(tmp_path / "nine.vcf")
    plfiles.write_vcf(p, SAMPLES, [nine])
    with pytest.raises(capi.NpsError) as e:
        host.GenotypeFile(p)
    assert "2:400" in str(e.value) and "9 alleles" in str(e.value)
    p = str(tmp_path / "nine.bcf")
    plfiles.write_bcf(p, ["2"], SAMPLES, [nine])
    with pytest.raises(capi.NpsError) as e:
        host.GenotypeFile(p)
    assert "2:400" in str(e.value) and "9 alleles" in str(e.value)
    # without the variable the same files are refused as before: no GT, no DS
    monkeypatch.delenv("NIMPRESS_FORMAT")
    with pytest.raises(capi.NpsError) as e:
        host.GenotypeFile(p)
    assert "without FORMAT/GT" in str(e.value)


# ------------------------------------------------------------------------------------------------------------------
# the readers alone, under sanitizers
def test_pl_readers_under_sanitizers(tmp_path):
    """tests/native/pl_driver.cpp (its own main; the reader units of build.HOST_READER_SOURCES, no libnps) built with
    -fsanitize=address,undefined on truncated PL fields, empty fields, a huge integer, short vectors, a wrong BCF length:
    a clean exit, no sanitizer report, the right values and the right refusals"""
    from nimpress_amd.build import HOST_READER_SOURCES
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "pl_driver")
    hostdir = os.path.join(ROOT, "nimpress_amd", "csrc", "host")
    # (-O0: the build is most of this test's time, and the sanitizers need no more)
    cmd = [gxx, "-O0", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "native", "pl_driver.cpp")] + [
               os.path.join(hostdir, f) for f in HOST_READER_SOURCES] + ["-lz"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    with open(exe, "rb") as f:      # the program IS instrumented: a clean run of a plain build would prove nothing
        image = f.read()
    assert b"__asan_init" in image and b"__ubsan_handle" in image
    head = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tA\tB\tC"]

    def text_file(name, body, newline=True):
        p = str(tmp_path / name)
        with open(p, "w") as f:
            f.write("\n".join(head + body) + ("\n" if newline else ""))
        return p

    ok = text_file("ok.vcf", [
        "1\t100\t.\tA\tG\t.\t.\t.\tGT:PL\t0/1:10,0,99999999999999999999\t0/0:0,3\t./.",            # huge, short, no PL subfield
        "1\t200\t.\tA\tG,T\t.\t.\t.\tGT:PL\t0/1:.\t0/0:\t1/2:1,2,3,4,5,6",                         # ".", empty, full
        "1\t300\t.\tA\tG\t.\t.\t.\tPL:GT\t0,.,7:0/1\t,:0/0\t2147483647,2147483648,0:1/1",           # PL first; int32 edge
        "1\t400\t.\tA\tG\t.\t.\t.\tGT\t0/1\t0/0\t1/1"])                                             # no PL: GT
    cut = text_file("cut.vcf", ["1\t100\t.\tA\tG\t.\t.\t.\tGT:PL\t0/1:10,0,9\t0/0:0,3"])            # a sample column short
    cut2 = text_file("cut2.vcf", ["1\t100\t.\tA\tG\t.\t.\t.\tGT:PL\t0/1:10,0,9\t0/0:0,3\t1/1:4,"], newline=False)
    long_ = text_file("long.vcf", ["1\t150\t.\tA\tG\t.\t.\t.\tGT:PL\t0/1:1,2,3,4\t0/0:0,3,4\t1/1:4,3,0"])
    nonint = text_file("nonint.vcf", ["1\t160\t.\tA\tG\t.\t.\t.\tGT:PL\t0/1:1,2,3\t0/0:0,-3,4\t1/1:4,3,0"])
    recs = make_records(False)
    lenbcf = str(tmp_path / "len.bcf")
    plfiles.write_bcf(lenbcf, ["1"], SAMPLES, [dict(recs[1], pl=recs[1]["pl"][:, :5])])
    okbcf = str(tmp_path / "ok.bcf")
    plfiles.write_bcf(okbcf, ["1", "2", "3"], SAMPLES, recs, pl_dtype=np.int16)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe, ok, cut, cut2, long_, nonint, lenbcf, okbcf], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    out = r.stdout.splitlines()
    assert "rec 1:100 src=PL per=3 bytes=4 pl=10,0,2147483647;0,3,E;M,M,M" in out
    assert "rec 1:200 src=PL per=6 bytes=4 pl=M,M,M,M,M,M;M,M,M,M,M,M;1,2,3,4,5,6" in out
    assert "rec 1:300 src=PL per=3 bytes=4 pl=0,M,7;M,M,E;2147483647,2147483647,0" in out
    assert "rec 1:400 src=GT per=0 bytes=0 pl=" in out
    refused = {ln.split(":", 1)[0].split()[1]: ln for ln in out if ln.startswith("refused ")}
    assert "too few sample columns" in refused[cut]
    assert cut2 not in refused and "rec 1:100 src=PL per=3 bytes=4 pl=10,0,9;0,3,E;4,M,E" in out   # "4," = 4, then an empty value
    assert "1:150" in refused[long_] and "more than 3 values" in refused[long_]
    assert "1:160" in refused[nonint] and "-3" in refused[nonint]
    assert "1:200" in refused[lenbcf] and "5 values" in refused[lenbcf] and "6 expected" in refused[lenbcf]
    # the good BCF: PL where the record has it and at most 8 alleles, the typed vector as it stands
    assert sum(ln.startswith("rec ") and "src=PL per=3 bytes=2" in ln for ln in out) == 3
    assert any(ln.startswith("rec 1:200 src=PL per=6 bytes=2") for ln in out)
    assert any(ln.startswith("rec 1:300 src=GT") for ln in out) and any(ln.startswith("rec 2:400 src=GT") for ln in out)
    want = ";".join(",".join("M" if x == M else ("E" if x == E else str(int(x))) for x in row) for row in recs[4]["pl"])
    assert "rec 2:500 src=PL per=3 bytes=2 pl=" + want in out
