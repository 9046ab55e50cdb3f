"""Test helper: writers of text VCF and BCF files whose records carry FORMAT/GT and FORMAT/PL (there is no htslib or
bcftools here; the BCF primitives are those of tests/bcfwriter.py).

A record is a dict: contig, pos (1-based), ref, alts (list), filters (list of names, [] = '.'), gts (int array
[n_samples, 2] in the BCF GT encoding, or None) and pl -- an int64 array [n_samples, G] of PL values in which PL_MISSING
stands for a missing value ('.' in text, the typed missing value in BCF) and PL_EOV for "no value" (the text vector ends
before it, BCF pads with end-of-vector) -- or None for a record without PL.  The number of columns is what a BCF record
declares per sample, whatever its alleles (a malformed record is written by passing too few columns)."""
import gzip
import struct

import numpy as np

import bcfwriter
from bcfwriter import bgzf_block, reg2bin, typed_desc, typed_int, typed_str

PL_MISSING, PL_EOV = -1, -2
_TYPED = {np.dtype(np.int8): (1, -128, -127), np.dtype(np.int16): (2, -32768, -32767),
          np.dtype(np.int32): (3, -2147483648, -2147483647)}


def typed_pl(pl, dtype) -> np.ndarray:
    """the record's PL array as the typed vector a BCF record of that width holds (what nps_push_pl is handed)"""
    dtype = np.dtype(dtype)
    _, miss, eov = _TYPED[dtype]
    pl = np.asarray(pl, dtype=np.int64)
    info = np.iinfo(dtype)
    assert pl.max() <= info.max, "PL value does not fit the width"
    out = np.where(pl == PL_MISSING, miss, np.where(pl == PL_EOV, eov, pl))
    return out.astype(dtype)


def gt_text(gts_row) -> str:
    al = [int(a) for a in gts_row if a != bcfwriter.INT32_END]
    sep = "|" if any(a & 1 for a in al[1:]) else "/"
    return sep.join("." if a < 2 else str((a >> 1) - 1) for a in al)


def pl_text(pl_row) -> str:
    vals = [int(x) for x in pl_row if x != PL_EOV]
    if not vals or all(x == PL_MISSING for x in vals):
        return "."
    return ",".join("." if x == PL_MISSING else str(x) for x in vals)


def vcf_lines(samples, records):
    out = ["##fileformat=VCFv4.2", '##FILTER=<ID=FAIL,Description="FAIL">',
           '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
           '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype likelihoods">',
           "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(samples)]
    for r in records:
        keys, cols = [], []
        if r.get("gts") is not None:
            keys.append("GT")
            cols.append([gt_text(g) for g in np.asarray(r["gts"])])
        if r.get("pl") is not None:
            keys.append("PL")
            cols.append([pl_text(p) for p in np.asarray(r["pl"])])
        cells = [":".join(c[i] for c in cols) for i in range(len(samples))]
        out.append("%s\t%d\t.\t%s\t%s\t.\t%s\t.\t%s\t%s" % (r["contig"], r["pos"], r["ref"], ",".join(r["alts"]) or ".",
                                                         ";".join(r.get("filters", [])) or ".", ":".join(keys),
                                                         "\t".join(cells)))
    return out


def write_vcf(path, samples, records):
    """plain text, or gzip when the path ends in .gz"""
    text = ("\n".join(vcf_lines(samples, records)) + "\n").encode()
    if path.endswith(".gz"):
        with gzip.open(path, "wb", compresslevel=1) as f:
            f.write(text)
    else:
        with open(path, "wb") as f:
            f.write(text)


def write_bcf(path, contigs, samples, records, gt_dtype=np.int8, pl_dtype=np.int16, with_csi=True, block_bytes=0xff00):
    """BCF2.2 (+ .csi): FORMAT/GT as gt_dtype, FORMAT/PL as pl_dtype vectors"""
    ids = ["PASS", "FAIL", "GT", "PL"]
    hdr = ["##fileformat=VCFv4.2", '##FILTER=<ID=PASS,Description="All filters passed">',
           '##FILTER=<ID=FAIL,Description="FAIL">'] + ["##contig=<ID=%s>" % c for c in contigs] + [
        '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
        '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype likelihoods">',
        "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(samples)]
    text = ("\n".join(hdr) + "\n").encode() + b"\0"
    gtype = _TYPED[np.dtype(gt_dtype)][0]
    gend = _TYPED[np.dtype(gt_dtype)][2]
    ptype = _TYPED[np.dtype(pl_dtype)][0]
    out, buf = bytearray(), bytearray()

    def flush():
        nonlocal buf
        if buf:
            out.extend(bgzf_block(bytes(buf)))
            buf = bytearray()

    def add(data: bytes):
        nonlocal buf
        start = (len(out) << 16) | len(buf)
        i = 0
        while i < len(data):
            room = block_bytes - len(buf)
            if room == 0:
                flush()
                room = block_bytes
            buf.extend(data[i:i + room])
            i += room
        if len(buf) >= block_bytes:
            flush()
        return start, (len(out) << 16) | len(buf)

    add(b"BCF\2\2" + struct.pack("<I", len(text)) + text)
    index = [dict() for _ in contigs]
    for r in records:
        chrom = contigs.index(r["contig"])
        pos0, rlen = r["pos"] - 1, len(r["ref"])
        alleles = [r["ref"]] + list(r["alts"])
        has_gt, has_pl = r.get("gts") is not None, r.get("pl") is not None
        shared = struct.pack("<iiiI", chrom, pos0, rlen, 0x7F800001)
        shared += struct.pack("<II", (len(alleles) << 16) | 0, ((int(has_gt) + int(has_pl)) << 24) | len(samples))
        shared += typed_str("")
        for a in alleles:
            shared += typed_str(a)
        fl = r.get("filters", [])
        shared += (typed_desc(len(fl), 1) + bytes(ids.index(f) for f in fl)) if fl else b"\x00"
        indiv = b""
        if has_gt:
            g = np.asarray(r["gts"], dtype=np.int64)
            g = np.where(g == bcfwriter.INT32_END, gend, g).astype(gt_dtype)
            indiv += typed_int(ids.index("GT")) + typed_desc(g.shape[1], gtype) + g.tobytes()
        if has_pl:
            p = typed_pl(r["pl"], pl_dtype)
            indiv += typed_int(ids.index("PL")) + typed_desc(p.shape[1], ptype) + p.tobytes()
        vs, ve = add(struct.pack("<II", len(shared), len(indiv)) + shared + indiv)
        index[chrom].setdefault(reg2bin(pos0, pos0 + rlen), []).append((vs, ve))
    flush()
    out.extend(bgzf_block(b""))
    with open(path, "wb") as f:
        f.write(bytes(out))
    if not with_csi:
        return
    t = bytearray(b"CSI\1" + struct.pack("<iii", 14, 5, 0) + struct.pack("<i", len(contigs)))
    for bins in index:
        t += struct.pack("<i", len(bins))
        for b, chunks in bins.items():
            t += struct.pack("<IQi", b, chunks[0][0], 1) + struct.pack("<QQ", chunks[0][0], chunks[-1][1])
    t += struct.pack("<Q", 0)
    tb = bytearray()
    for i in range(0, len(t), 0xff00):
        tb += bgzf_block(bytes(t[i:i + 0xff00]))
    tb += bgzf_block(b"")
    with open(path + ".csi", "wb") as f:
        f.write(bytes(tb))


def write_score(path, rows, offset=0.0, name="pl-test"):
    """rows: (contig, pos, ref, ea, beta, eaf)"""
    with open(path, "w") as f:
        f.write("%s\n\n\nx\n%r\n" % (name, offset))
        for c, p, ref, ea, beta, eaf in rows:
            f.write("%s\t%d\t%s\t%s\t%r\t%s\n" % (c, p, ref, ea, beta, "NaN" if eaf != eaf else repr(eaf)))
