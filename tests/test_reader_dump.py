"""What the genotype file readers hand out, field by field and refusal by refusal, pinned to a recorded expectation.

tests/native/reader_dump.cpp (its own main, the reader units alone, no libnps) opens a small corpus written here -- text
VCF, BCF, vcf.gz + .tbi, BCF + .csi, PLINK filesets, good files and one file per refusal -- and prints every field of
every Variant, or the reader's message.  tests/reader_dump_expected.txt is that output as the readers stood BEFORE their
copies were collapsed and the unit was split (DESIGN.md section 9, f1 names the commit and the command); the whole output
must equal it, in a plain build and in a -fsanitize=address,undefined build that leaves no report.  Nothing here is
random: the text is literal, the binary files come from tests/bcfwriter.py, tests/plfiles.py and tests/pgenwriter.py.

To record again (only ever from a tree whose readers are known good):  python tests/test_reader_dump.py --record"""
import gzip
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import bcfwriter  # noqa: E402
import pgenwriter  # noqa: E402
import plfiles  # noqa: E402
from bcfwriter import typed_desc, typed_int, typed_str  # noqa: E402
from tbiwriter import write_bgzf_vcf_with_tbi  # noqa: E402

EXPECTED = os.path.join(ROOT, "tests", "reader_dump_expected.txt")
HOSTDIR = os.path.join(ROOT, "nimpress_amd", "csrc", "host")
COLS = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"
HEAD = ["##fileformat=VCFv4.2", COLS + "\tFORMAT\tA\tB\tC"]
E = bcfwriter.INT32_END


def reader_sources():
    """the units that link without libnps (nimpress_amd/build.py)"""
    from nimpress_amd import build
    return [os.path.join(HOSTDIR, f) for f in build.HOST_READER_SOURCES]


def rec(pos, ref, alt, fmt, *cells, contig="1", id_=".", filt="."):
    return "\t".join([contig, str(pos), id_, ref, alt, ".", filt, ".", fmt] + list(cells))


# ---- text VCF -------------------------------------------------------------------------------------------------------
GOOD = [
    rec(100, "A", "G", "GT", "0/1", "1|0", "./.", id_="rs1", filt="PASS"),            # phased, unphased, ./.
    rec(200, "AC", "G,T", "GT:DP", "0:3", "0/1/2:4", ".:5", filt="q10;s50"),          # haploid + triploid: vector-end pads
    rec(300, "A", "G", "GT", "0/64", "63|0", "0/0"),                                  # allele index above 63: int32 gts
    rec(400, "A", "G", "DP:GT", "3:", "4:0/1", "5"),                                  # an empty and an absent sub-field
    rec(500, "A", "G", "GT:DS", "0/1:1.0", "1/1:1.95", "./.:.", filt="PASS"),         # GT and DS
    rec(600, "A", "G", "DS", "0.5", ".", "2"),                                        # DS only
    rec(800, "A", "G,T", "GT:DS", "0/1:0.9,0.1", "1/2:1", "0/0:.,0.2"),               # Number=A, a short list, "." inside
    rec(900, "A", "G", "GT:PL", "0/1:10,0", "0/0:0,.,7", "1/1:99999999999,3,0"),      # PL short, "." inside, beyond int32
    rec(1000, "A", ".", "GT:PL", "0/0:0", "0/0:0", "0/0:0"),                          # ALT ".": one allele, never PL
    rec(150, "A", "G", "GT:DS:PL", "1/1:2:30,20,0", "0/1:1:9,0,9", "0/0:0:0,5,50", contig="2"),
]
PL_ONLY = [
    rec(700, "A", "G", "PL", "0,10,20", ".", "30,0"),                                 # PL only
    rec(750, "A", "C,G,T,AA,AC,AG,AT,CA", "GT:PL", "0/8:1,2", "0/0:0", "./.:."),       # 9 alleles: PL is passed over for GT
]
REFUSED_TEXT = [  # (file, format, record lines): one file per message
    ("cols7", "-", ["1\t100\t.\tA\tG\t.\tPASS"]),
    ("nocols", "-", ["1\t100\t.\tA\tG\t.\tPASS\t."]),
    ("few_gt", "-", [rec(100, "A", "G", "GT", "0/1", "0/0")]),
    ("few_ds", "-", [rec(100, "A", "G", "DS", "0.5", "1")]),
    ("few_pl", "PL", [rec(100, "A", "G", "GT:PL", "0/1:10,0,9", "0/0:0,3")]),
    ("bad_gt", "-", [rec(100, "A", "G", "GT", "0/1", "0/x", "1/1")]),
    ("ploidy9", "-", [rec(100, "A", "G", "GT", "0/1", "0/0/0/0/0/0/0/0/0", "1/1")]),
    ("no_gt_ds", "-", [rec(100, "A", "G", "GT", "0/1", "0/0", "1/1"), rec(125, "A", "G", "DP", "1", "2", "3")]),
    ("pl_many", "PL", [rec(150, "A", "G", "GT:PL", "0/1:1,2,3,4", "0/0:0,3,4", "1/1:4,3,0")]),
    ("pl_nonint", "PL", [rec(160, "A", "G", "GT:PL", "0/1:1,2,3", "0/0:0,-3,4", "1/1:4,3,0")]),
    ("pl_nine", "PL", [rec(170, "A", "C,G,T,AA,AC,AG,AT,CA", "PL", "0", "0", "0")]),
    ("ds_junk", "-", [rec(100, "A", "G", "DS", "0.5", "1.5x", "1")]),
    ("ds_long", "-", [rec(100, "A", "G", "DS", "0.5", "0." + "1" * 80, "1")]),
    ("ds_inf", "-", [rec(100, "A", "G", "GT:DS", "0/1:0.5", "0/0:inf", "1/1:1")]),   # (GT wins: read)
    ("ds_inf", "DS", None),
    ("early", "-", None),
]
SCORE_ROWS = [("1", 100, "A", "G"), ("1", 201, "C", "T"), ("1", 500, "A", "G"), ("1", 800, "A", "T"), ("1", 900, "A", "G"),
              ("1", 20000, "A", "G"), ("2", 150, "A", "G"), ("3", 10, "A", "G"), ("2", 300, "AT", "A")]


def write_text(path, lines, newline="\n"):
    with open(path, "w", newline="") as f:
        f.write(newline.join(lines) + newline)


# ---- BCF ------------------------------------------------------------------------------------------------------------
def gt(*rows):
    """rows of allele indices (None = missing, short rows padded) -> the BCF GT encoding"""
    width = max(len(r) for r in rows)
    return np.array([[(0 if a is None else (a + 1) << 1) for a in r] + [E] * (width - len(r)) for r in rows], np.int64)


def bcf_records():
    nan = float("nan")
    ds800 = np.array([[0.9, 0.1], [1.0, 0.0], [nan, 0.2]], np.float32)
    ds800.view(np.uint32)[1, 1] = 0x7F800002                            # a short list: end of vector
    return [
        dict(contig="1", pos=100, id="rs1", ref="A", alts=["G"], filters=["PASS"], gts=gt((0, 1), (1, 0), (None, None))),
        dict(contig="1", pos=200, id=".", ref="AC", alts=["G", "T"], filters=["q10", "s50"], gts=gt((0,), (0, 1, 2), (None,))),
        dict(contig="1", pos=500, id=".", ref="A", alts=["G"], filters=[], gts=gt((0, 1), (1, 1), (None, None)),
             ds=[[1.0], [1.95], [nan]]),
        dict(contig="1", pos=600, id=".", ref="A", alts=["G"], filters=[], gts=None, ds=[[0.5], [nan], [2.0]]),
        dict(contig="1", pos=800, id=".", ref="A", alts=["G", "T"], filters=[], gts=gt((0, 1), (1, 2), (0, 0)),
             ds=ds800),
        dict(contig="1", pos=20000, id=".", ref="A", alts=["G"], filters=["PASS"], gts=gt((1, 1), (0, 0), (0, 1))),
        dict(contig="2", pos=150, id=".", ref="A", alts=["G"], filters=[], gts=gt((1, 1), (0, 1), (0, 0))),
        dict(contig="2", pos=299, id=".", ref="CAT", alts=["C"], filters=[], gts=gt((0, 1), (0, 0), (1, 1))),
    ]


def pl_records():
    M, V = plfiles.PL_MISSING, plfiles.PL_EOV
    return [
        dict(contig="1", pos=100, ref="A", alts=["G"], filters=[], gts=gt((0, 1), (0, 0), (1, 1)),
             pl=np.array([[10, 0, 120], [0, M, 7], [M, M, M]])),
        dict(contig="1", pos=800, ref="A", alts=["G", "T"], filters=["FAIL"], gts=gt((0, 1), (1, 2), (0, 0)),
             pl=np.array([[1, 2, 3, 4, 5, 6], [0, 3, V, V, V, V], [9, 8, 7, 6, 5, 0]])),
        dict(contig="2", pos=150, ref="A", alts=["G"], filters=[], gts=gt((0, 1), (0, 0), (1, 1)), pl=None),
        dict(contig="2", pos=300, ref="AT", alts=["A"], filters=[], gts=None, pl=np.array([[0, 1, 2], [3, 0, 3], [2, 1, 0]])),
    ]


def raw_bcf(path, samples, records, cut=0, magic=b"BCF\2\2"):
    """an uncompressed BCF assembled by hand, for what bcfwriter does not write.  records: (chrom, pos0, rlen, alleles,
    filter bytes, n_sample, [(key, typed vector bytes)]); dictionary: PASS 0, q10 1, GT 2, DS 3, PL 4."""
    hdr = ["##fileformat=VCFv4.2", '##FILTER=<ID=PASS,Description="All filters passed">', '##FILTER=<ID=q10,Description="q">',
           "##contig=<ID=1>", "##contig=<ID=2>", '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
           '##FORMAT=<ID=DS,Number=A,Type=Float,Description="ALT allele dosage">',
           '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="PL">', "\t".join([COLS] + (["FORMAT"] + samples if samples else []))]
    text = ("\n".join(hdr) + "\n").encode() + b"\0"
    out = magic + struct.pack("<I", len(text)) + text
    for chrom, pos0, rlen, alleles, filt, n_sample, fmt in records:
        shared = struct.pack("<iiiI", chrom, pos0, rlen, 0x7F800001)
        shared += struct.pack("<II", len(alleles) << 16, (len(fmt) << 24) | n_sample) + typed_str("")
        shared += b"".join(typed_str(a) for a in alleles) + filt
        indiv = b"".join(typed_int(key) + vec for key, vec in fmt)
        out += struct.pack("<II", len(shared), len(indiv)) + shared + indiv
    with open(path, "wb") as f:
        f.write(out[:len(out) - cut])


GT8 = (2, typed_desc(2, 1) + bytes([2, 4, 4, 4, 0, 0]))                               # 0/1 1/1 ./. as int8
DS_F = (3, typed_desc(1, 5) + np.array([1.0, 2.0, 0.5], np.float32).tobytes())
DS_I = (3, typed_desc(1, 1) + bytes([1, 2, 0]))
PL8 = (4, typed_desc(3, 1) + bytes([0, 10, 20, 10, 0, 10, 20, 10, 0]))
REFUSED_BCF = [  # (file, formats, samples, records, kwargs)
    ("chrom", ["-"], 3, [(2, 99, 1, ["A", "G"], b"\x00", 3, [GT8])], {}),
    ("filter", ["-"], 3, [(0, 99, 1, ["A", "G"], typed_desc(1, 1) + b"\x09", 3, [GT8])], {}),
    ("gt_float", ["-"], 3, [(0, 99, 1, ["A", "G"], b"\x00", 3, [(2, DS_F[1])])], {}),
    ("ds_int", ["-", "DS"], 3, [(0, 99, 1, ["A", "G"], b"\x00", 3, [GT8, DS_I])], {}),   # ignored under GT, refused under DS
    ("ds_empty", ["-"], 3, [(0, 99, 1, ["A", "G"], b"\x00", 3, [(3, typed_desc(0, 5))])], {}),
    ("pl_len", ["PL"], 3, [(0, 99, 1, ["A", "G", "T"], b"\x00", 3, [GT8, PL8])], {}),
    ("pl_float", ["PL", "-"], 3, [(0, 99, 1, ["A", "G"], b"\x00", 3, [GT8, (4, typed_desc(3, 5) + bytes(36))])], {}),
    ("pl_nine", ["PL"], 3, [(0, 99, 1, ["A", "C", "G", "T", "AA", "AC", "AG", "AT", "CA"], b"\x00", 3, [PL8])], {}),
    ("no_gt_ds", ["-"], 3, [(0, 99, 1, ["A", "G"], b"\x00", 3, [PL8])], {}),
    ("nsample", ["-"], 3, [(0, 99, 1, ["A", "G"], b"\x00", 2, [GT8])], {}),
    ("cut", ["-"], 3, [(0, 99, 1, ["A", "G"], b"\x00", 3, [GT8]), (0, 199, 1, ["A", "G"], b"\x00", 3, [GT8])], dict(cut=5)),
    ("magic", ["-"], 3, [(0, 99, 1, ["A", "G"], b"\x00", 3, [GT8])], dict(magic=b"BCF\1\2")),
    ("zero", ["-", "PL"], 0, [(0, 99, 1, ["A", "G"], typed_desc(2, 1) + b"\x00\x01", 0, []),      # no samples: no format rule
                              (1, 9, 2, ["AT", "A"], b"\x00", 0, [])], {}),
]


# ---- the corpus -----------------------------------------------------------------------------------------------------
def write_corpus(d):
    """writes every file into directory d; returns the driver's arguments (paths relative to d) and the indices of those
    that go through the parallel indexed fetch"""
    args = []

    def p(name):
        return os.path.join(d, name)

    with open(p("rows.score"), "w") as f:
        f.write("dump\n\n\nx\n0.0\n" + "".join("%s\t%d\t%s\t%s\t0.1\t0.2\n" % r for r in SCORE_ROWS))
    write_text(p("good.vcf"), HEAD + GOOD)
    write_text(p("crlf.vcf"), HEAD + GOOD[:3], newline="\r\n")
    with open(p("last.vcf"), "w") as f:                                   # the last line unterminated
        f.write("\n".join(HEAD + GOOD[:2]))
    with open(p("good.vcf.gz"), "wb") as f:
        f.write(gzip.compress(("\n".join(HEAD + GOOD) + "\n").encode(), mtime=0))
    write_text(p("pl_only.vcf"), HEAD + PL_ONLY)
    write_text(p("nosamples.vcf"), [HEAD[0], COLS, "1\t100\trs1\tA\tG\t.\tPASS\t.", "1\t200\t.\tAC\t.\t.\t.\t."])
    args += ["-:scan:good.vcf", "DS:scan:good.vcf", "PL:scan:good.vcf", "-:keep:good.vcf", "-:stream1:good.vcf",
             "-:scan:crlf.vcf", "-:scan:last.vcf", "DS:keep:good.vcf.gz", "PL:scan:pl_only.vcf", "-:scan:pl_only.vcf",
             "-:scan:nosamples.vcf", "-:keep:nosamples.vcf", "-:scan:absent.vcf"]
    for name, fmt, lines in REFUSED_TEXT:
        if name == "early":
            write_text(p("early.vcf"), [HEAD[0], GOOD[0], HEAD[1]])
        elif lines is not None:
            write_text(p(name + ".vcf"), HEAD + lines)
        args.append("%s:scan:%s.vcf" % (fmt, name))

    # BCF, whole-file scan: GT as int8 / int16 / int32, DS, a FILTER list of two ids, an empty ID; PL as int8 / int16
    for tag, dt in (("8", np.int8), ("16", np.int16), ("32", np.int32)):
        bcfwriter.write_bcf(p("gt%s.bcf" % tag), ["1", "2"], ["A", "B", "C"], bcf_records(), gt_dtype=dt,
                            filters=("PASS", "q10", "s50"), with_csi=False)
        args += ["-:scan:gt%s.bcf" % tag]
    args += ["DS:scan:gt8.bcf", "-:keep:gt16.bcf"]
    for tag, dt in (("8", np.int8), ("16", np.int16)):
        plfiles.write_bcf(p("pl%s.bcf" % tag), ["1", "2"], ["A", "B", "C"], pl_records(), pl_dtype=dt, with_csi=False)
        args += ["PL:scan:pl%s.bcf" % tag]
    args += ["-:scan:pl8.bcf"]
    for name, fmts, ns, records, kw in REFUSED_BCF:
        raw_bcf(p(name + ".bcf"), ["A", "B", "C"][:ns], records, **kw)
        args += ["%s:scan:%s.bcf" % (f, name) for f in fmts]

    # indexed: many small BGZF blocks, two contigs, score rows that share an index chunk, a contig the file lacks, a
    # multi-base REF reaching a row from the left; a truncated index
    indexed = []
    vrecs = [("1", 100, "A", GOOD[0]), ("1", 200, "AC", GOOD[1]), ("1", 500, "A", GOOD[4]), ("1", 600, "A", GOOD[5]),
             ("1", 800, "A", GOOD[6]), ("1", 900, "A", GOOD[7]),
             ("1", 20000, "A", rec(20000, "A", "G", "GT", "1/1", "0/0", "0/1", filt="PASS")),
             ("2", 150, "A", GOOD[9]), ("2", 299, "CAT", rec(299, "CAT", "C", "GT", "0/1", "0/0", "1/1", contig="2"))]
    write_bgzf_vcf_with_tbi(p("ix.vcf.gz"), HEAD, vrecs, block_bytes=150)
    bcfwriter.write_bcf(p("ix.bcf"), ["1", "2"], ["A", "B", "C"], bcf_records(), gt_dtype=np.int8,
                        filters=("PASS", "q10", "s50"), block_bytes=150)
    plfiles.write_bcf(p("ixpl.bcf"), ["1", "2"], ["A", "B", "C"], pl_records(), pl_dtype=np.int8, block_bytes=150)
    for a in ("-:keep:ix.vcf.gz", "-:stream1:ix.vcf.gz", "DS:stream2:ix.vcf.gz", "PL:stream2:ix.vcf.gz", "-:scan:ix.vcf.gz",
              "-:keep:ix.bcf", "DS:stream1:ix.bcf", "-:stream2:ix.bcf", "-:scan:ix.bcf", "PL:keep:ixpl.bcf",
              "PL:stream2:ixpl.bcf"):
        if ":scan:" not in a:
            indexed.append(len(args))
        args.append(a)
    for src, ext in (("ix.vcf.gz", ".tbi"), ("ix.bcf", ".csi")):
        name = "trunc" + src[2:]
        shutil.copy(p(src), p(name))
        payload = gzip.decompress(open(p(src + ext), "rb").read())
        with open(p(name + ext), "wb") as f:
            f.write(gzip.compress(payload[:len(payload) - 11], mtime=0))
        args += ["-:keep:" + name, "-:stream1:" + name]
    with open(p("cutfile.vcf.gz"), "wb") as f:                            # the data file itself cut inside a block
        raw = open(p("ix.vcf.gz"), "rb").read()
        f.write(raw[:len(raw) * 2 // 3])
    shutil.copy(p("ix.vcf.gz.tbi"), p("cutfile.vcf.gz.tbi"))
    with open(p("cutfile.bcf"), "wb") as f:
        raw = open(p("ix.bcf"), "rb").read()
        f.write(raw[:len(raw) * 2 // 3])
    shutil.copy(p("ix.bcf.csi"), p("cutfile.bcf.csi"))
    args += ["-:keep:cutfile.vcf.gz", "-:keep:cutfile.bcf"]

    # PLINK: a .bed fileset, a fixed-width .pgen, and what is refused
    with open(p("b.bed"), "wb") as f:                                     # 5 samples: two bytes per variant
        f.write(bytes([0x6c, 0x1b, 0x01, 0b11100100, 0b01, 0b00011011, 0b10, 0b10101010, 0b11]))
    write_text(p("b.bim"), ["1\trs1\t0\t100\tG\tA", "1 v2 0 200 G AC", "2\tv3\t0\t150\tA\tG"])
    write_text(p("b.fam"), ["F%d I%d 0 0 0 -9" % (k, k) for k in range(5)])
    variants = [("1", 100, "rs1", "A", "G"), ("1", 200, "v2", "AC", "G"), ("2", 150, "v3", "A", "G"), ("2", 300, "v4", "AT", "A")]
    alt = np.array([[0, 1, 2, 0, 1], [2, 2, 0, 0, 1], [1, 0, 0, 2, 2], [0, 0, 1, 1, 2]])
    miss = np.array([[0, 0, 0, 1, 0], [0, 0, 0, 0, 0], [1, 0, 0, 0, 0], [0, 0, 0, 0, 1]], bool)
    pgenwriter.write_pgen(p("g"), ["I%d" % k for k in range(5)], variants, alt, miss)
    pgenwriter.write_pgen(p("h"), ["I%d" % k for k in range(5)], variants, alt, miss, pvar_header=False, psam_fid=True)
    for name, mode in (("major", 0), ("mode", 0x10)):
        with open(p(name + (".bed" if mode == 0 else ".pgen")), "wb") as f:
            f.write(bytes([0x6c, 0x1b, mode, 0, 0, 0, 0]))
    shutil.copy(p("b.bed"), p("fam.bed"))
    shutil.copy(p("b.bim"), p("fam.bim"))
    write_text(p("fam.fam"), ["F0 I0 0 0 0 -9", "F1"])
    args += ["-:scan:b.bed", "-:keep:b.bed", "-:stream1:b.bed", "-:scan:g.pgen", "-:keep:g.pgen", "-:scan:h.pgen",
             "-:scan:major.bed", "-:scan:mode.pgen", "-:scan:fam.bed"]
    return args, indexed


def build_driver(exe, extra):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    cmd = [gxx, "-std=c++17", "-pthread"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "native", "reader_dump.cpp")
                                                      ] + reader_sources() + ["-lz"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]


def run_driver(exe, d, args, threads):
    env = dict(os.environ, NIMPRESS_THREADS=str(threads), ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("NIMPRESS_NO_INDEX", None)
    r = subprocess.run([exe, "rows.score"] + args, capture_output=True, text=True, env=env, cwd=d)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return r


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("reader_dump"))
    args, indexed = write_corpus(d)
    return d, args, indexed


def check_output(out):
    with open(EXPECTED) as f:
        want = f.read()
    if out != want:                                                        # the first differing line says where to look
        a, b = out.splitlines(), want.splitlines()
        k = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
        sect = [ln for ln in a[:k + 1] if ln.startswith("== ")]
        pytest.fail("reader output differs from tests/reader_dump_expected.txt at line %d (%s)\n  got:  %s\n  want: %s" % (
            k + 1, sect[-1] if sect else "?", a[k] if k < len(a) else "<end>", b[k] if k < len(b) else "<end>"))


def test_reader_dump_equals_the_recorded_expectation(corpus, tmp_path):
    """every Variant field and every refusal of the corpus equals the recording; the indexed fetches give the same lines
    with three fetch threads as with one"""
    d, args, indexed = corpus
    exe = str(tmp_path / "reader_dump")
    build_driver(exe, ["-O1"])
    out = run_driver(exe, d, args, 1).stdout
    check_output(out)
    sub = [args[k] for k in indexed]
    assert run_driver(exe, d, sub, 3).stdout == run_driver(exe, d, sub, 1).stdout


def test_reader_dump_under_sanitizers(corpus, tmp_path):
    """the same driver built with -fsanitize=address,undefined (a stand-alone program): the same output, no report"""
    d, args, indexed = corpus
    exe = str(tmp_path / "reader_dump_san")
    # (-O0: the build is most of this test's time, and the sanitizers need no more)
    # (the sanitizer runtimes linked statically: a stand-alone program that asks nothing of the environment it starts in)
    build_driver(exe, ["-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                       "-static-libasan", "-static-libubsan"])
    with open(exe, "rb") as f:      # the program IS instrumented: a clean run of a plain build would prove nothing
        image = f.read()
    assert b"__asan_init" in image and b"__ubsan_handle" in image
    for threads, sub in ((1, args), (3, [args[k] for k in indexed])):
        r = run_driver(exe, d, sub, threads)
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        if threads == 1:
            check_output(r.stdout)


if __name__ == "__main__":
    # python tests/test_reader_dump.py --record [reader sources ...]: writes the expectation from a plain build of the
    # driver against the given reader sources (default: this tree's)
    import tempfile
    assert sys.argv[1] == "--record"
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, "corpus")
        os.mkdir(d)
        args, _ = write_corpus(d)
        exe = os.path.join(tmp, "reader_dump")
        if sys.argv[2:]:
            reader_sources = lambda: [os.path.abspath(s) for s in sys.argv[2:]]  # noqa: E731
        build_driver(exe, ["-O1"])
        with open(EXPECTED, "w") as f:
            f.write(run_driver(exe, d, args, 1).stdout)
    print("recorded", EXPECTED)
