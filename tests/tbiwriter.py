"""Test helper: a BGZF text VCF with its tabix (.tbi) index, to exercise multi-block random access (there is no htslib
or tabix here).  The twin of tests/bcfwriter.py, whose BGZF block and bin number it uses."""
import struct

from bcfwriter import bgzf_block, reg2bin


def write_bgzf_vcf_with_tbi(path, header_lines, records, block_bytes=0xff00):
    """records: list of (contig, pos, ref, line) sorted by contig order of appearance, pos.  block_bytes: the text held by
    one BGZF block (a small value makes a small file span many blocks)."""
    out = bytearray()
    buf = bytearray()
    voffs = []

    def flush():
        nonlocal buf
        if buf:
            out.extend(bgzf_block(bytes(buf)))
            buf = bytearray()

    def add_line(txt):
        nonlocal buf
        data = txt.encode() + b"\n"
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
        end = (len(out) << 16) | len(buf)
        return start, end

    for h in header_lines:
        add_line(h)
    contigs = []
    index = {}
    for contig, pos, ref, line in records:
        vs, ve = add_line(line)
        if contig not in index:
            contigs.append(contig)
            index[contig] = ({}, {})
        bins, lin = index[contig]
        beg, end = pos - 1, pos - 1 + len(ref)
        bins.setdefault(reg2bin(beg, end), []).append((vs, ve))
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            lin[w] = min(lin.get(w, vs), vs)
    flush()
    out.extend(bgzf_block(b""))
    open(path, "wb").write(bytes(out))
    names = b"".join(c.encode() + b"\0" for c in contigs)
    t = bytearray(b"TBI\1" + struct.pack("<8i", len(contigs), 2, 1, 2, 0, ord("#"), 0, len(names)) + names)
    for c in contigs:
        bins, lin = index[c]
        t += struct.pack("<i", len(bins))
        for b, chunks in bins.items():
            merged = [(chunks[0][0], chunks[-1][1])]
            t += struct.pack("<Ii", b, len(merged))
            for vs, ve in merged:
                t += struct.pack("<QQ", vs, ve)
        nw = max(lin) + 1 if lin else 0
        t += struct.pack("<i", nw)
        last = 0
        for w in range(nw):
            last = lin.get(w, last)
            t += struct.pack("<Q", last)
    tb = bytearray()
    for i in range(0, len(t), 0xff00):
        tb += bgzf_block(bytes(t[i:i + 0xff00]))
    tb += bgzf_block(b"")
    open(path + ".tbi", "wb").write(bytes(tb))
