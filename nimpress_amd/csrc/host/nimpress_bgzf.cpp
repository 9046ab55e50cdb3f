// nimpress_bgzf.cpp -- see nimpress_readers.hpp.  Inflate of a whole gzip / BGZF buffer, BGZF random access by virtual
// offset, and the bin index of tabix and CSI files: what hts-nim's vcf.query() does through htslib.
#include "nimpress_readers.hpp"

#include <zlib.h>

#include <algorithm>
#include <limits>

namespace nimpress {

bool inflateAll(const std::string &in, std::string &out) {
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, 15 + 32) != Z_OK) return false;  // gzip or zlib header, auto-detected
    zs.next_in = (Bytef *)in.data();
    zs.avail_in = (uInt)std::min<size_t>(in.size(), std::numeric_limits<uInt>::max());
    size_t consumed_total = 0;
    std::vector<char> buf(1 << 20);
    out.clear();
    while (true) {
        zs.next_out = (Bytef *)buf.data();
        zs.avail_out = (uInt)buf.size();
        const int rc = inflate(&zs, Z_NO_FLUSH);
        out.append(buf.data(), buf.size() - zs.avail_out);
        if (rc == Z_STREAM_END) {
            // BGZF = concatenated gzip members: continue with the next one if input remains
            consumed_total = in.size() - zs.avail_in;
            if (consumed_total >= in.size()) break;
            if (inflateReset(&zs) != Z_OK) {
                inflateEnd(&zs);
                return false;
            }
            continue;
        }
        if (rc != Z_OK) {
            inflateEnd(&zs);
            return false;
        }
        if (zs.avail_in == 0 && zs.avail_out != 0) break;  // truncated input: keep what we have
    }
    inflateEnd(&zs);
    return true;
}

// ---- BGZF random access ----------------------------------------------------------------------------------------------
bool BgzfFile::open(const std::string &path) {
    f = fopen(path.c_str(), "rb");
    return f != nullptr;
}

// inflate the BGZF block starting at compressed offset `coff`; returns false at EOF / on error
bool BgzfFile::block(uint64_t coff, const std::string **data, uint32_t *csize) {
    auto it = cache.find(coff);
    if (it == cache.end()) {
        unsigned char hdr[18];
        if (fseeko(f, (off_t)coff, SEEK_SET) != 0 || fread(hdr, 1, 18, f) != 18) return false;
        if (hdr[0] != 0x1f || hdr[1] != 0x8b || !(hdr[3] & 4)) return false;
        const unsigned xlen = hdr[10] | (hdr[11] << 8);
        std::vector<unsigned char> extra(xlen);
        if (fseeko(f, (off_t)coff + 12, SEEK_SET) != 0 || fread(extra.data(), 1, xlen, f) != xlen)
            return false;
        int bsize = -1;
        for (unsigned i = 0; i + 4 <= xlen;) {
            const unsigned slen = extra[i + 2] | (extra[i + 3] << 8);
            if (extra[i] == 'B' && extra[i + 1] == 'C' && slen == 2)
                bsize = (extra[i + 4] | (extra[i + 5] << 8)) + 1;
            i += 4 + slen;
        }
        if (bsize < 0) return false;  // a plain gzip file, not BGZF
        const unsigned cdata = (unsigned)bsize - xlen - 12 - 8;
        std::vector<unsigned char> comp(cdata + 8);
        if (fread(comp.data(), 1, cdata + 8, f) != cdata + 8) return false;
        const uint32_t isize = comp[cdata + 4] | (comp[cdata + 5] << 8) | (comp[cdata + 6] << 16) |
                               ((uint32_t)comp[cdata + 7] << 24);
        std::string out(isize, '\0');
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        if (inflateInit2(&zs, -15) != Z_OK) return false;
        zs.next_in = comp.data();
        zs.avail_in = cdata;
        zs.next_out = (Bytef *)out.data();
        zs.avail_out = isize;
        const int rc = inflate(&zs, Z_FINISH);
        inflateEnd(&zs);
        if (rc != Z_STREAM_END) return false;
        if (cache.size() > 64) cache.clear();
        it = cache.emplace(coff, std::make_pair(std::move(out), (uint32_t)bsize)).first;
    }
    *data = &it->second.first;
    *csize = it->second.second;
    return true;
}

// On to the start of the block behind block `d` (csize compressed bytes at a.coff).  An empty block -- the EOF marker --
// is only stepped over if a block follows it: false, and `a` as it was, otherwise.  (`d` may be gone afterwards.)
bool BgzfFile::advance(At &a, const std::string &d, uint32_t csize) {
    if (d.empty()) {
        const std::string *d2;
        uint32_t c2;
        if (!block(a.coff + csize, &d2, &c2)) return false;
    }
    a.coff += csize;
    a.uoff = 0;
    return true;
}

bool BgzfFile::readBytes(uint64_t *voff, void *dst, size_t n) {
    At a{*voff >> 16, (uint32_t)(*voff & 0xffff)};
    char *out = (char *)dst;
    while (n) {
        const std::string *d;
        uint32_t csize;
        if (!block(a.coff, &d, &csize)) return false;
        if (a.uoff < d->size()) {
            const size_t take = std::min(n, d->size() - a.uoff);
            memcpy(out, d->data() + a.uoff, take);
            out += take;
            n -= take;
            a.uoff += (uint32_t)take;
        }
        if (a.uoff >= d->size() && !advance(a, *d, csize)) return false;
    }
    *voff = (a.coff << 16) | a.uoff;
    return true;
}

bool BgzfFile::readLine(uint64_t *voff, std::string &line) {
    line.clear();
    At a{*voff >> 16, (uint32_t)(*voff & 0xffff)};
    while (true) {
        const std::string *d;
        uint32_t csize;
        if (!block(a.coff, &d, &csize)) return !line.empty();
        const char *b = d->data() + a.uoff, *e = d->data() + d->size();
        const char *nl = d->empty() ? nullptr : (const char *)memchr(b, '\n', (size_t)(e - b));
        if (nl) {
            line.append(b, nl - b);
            a.uoff = (uint32_t)(nl + 1 - d->data());
            if (a.uoff >= d->size()) advance(a, *d, csize);
            *voff = (a.coff << 16) | a.uoff;
            if (!line.empty() && line.back() == '\r') line.pop_back();
            return true;
        }
        if (!d->empty()) line.append(b, e - b);
        if (!advance(a, *d, csize)) return !line.empty();  // the EOF marker with nothing behind it
    }
}

// ---- the bin index -----------------------------------------------------------------------------------------------------
namespace {
struct IndexCursor {  // little-endian values off the inflated index; `kind` (".tbi" / ".csi") names the file in the message
    const std::string &t;
    size_t o;
    const char *kind;
    template <class T> T get() {
        T v;
        if (o + sizeof v > t.size()) throw std::runtime_error(std::string("truncated ") + kind);
        memcpy(&v, t.data() + o, sizeof v);
        o += sizeof v;
        return v;
    }
    int32_t i32() { return get<int32_t>(); }
    uint64_t u64() { return get<uint64_t>(); }
};
}  // namespace

bool BinIndex::load(const std::string &path, bool is_tabix) {
    std::string raw, t;
    if (!readFile(path, raw) || !inflateAll(raw, t)) return false;
    tabix = is_tabix;
    if (t.size() < (tabix ? 36u : 16u) || memcmp(t.data(), tabix ? "TBI\1" : "CSI\1", 4) != 0) return false;
    IndexCursor c{t, 4, tabix ? ".tbi" : ".csi"};
    int32_t n_ref;
    if (tabix) {
        n_ref = c.i32();
        for (int k = 0; k < 6; ++k) (void)c.i32();  // format, col_seq, col_beg, col_end, meta, skip
        const int32_t l_nm = c.i32();
        for (size_t a = c.o; a < c.o + (size_t)l_nm;) {
            const char *name = t.data() + a;
            names.emplace_back(name);
            a += names.back().size() + 1;
        }
        c.o += (size_t)l_nm;
    } else {
        min_shift = c.i32();
        depth = c.i32();
        const int32_t l_aux = c.i32();
        if (l_aux < 0 || c.o + (size_t)l_aux > t.size()) throw std::runtime_error("truncated .csi");
        c.o += (size_t)l_aux;
        n_ref = c.i32();
    }
    refs.resize((size_t)std::max(n_ref, 0));
    for (int32_t r = 0; r < n_ref; ++r) {
        Ref &ref = refs[(size_t)r];
        const int32_t n_bin = c.i32();
        for (int32_t b = 0; b < n_bin; ++b) {
            const uint32_t bin = (uint32_t)c.i32();
            if (!tabix) (void)c.u64();  // loffset: not used
            const int32_t n_chunk = c.i32();
            Chunks &v = ref.bins[bin];
            for (int32_t k = 0; k < n_chunk; ++k) {
                const uint64_t beg = c.u64(), end = c.u64();
                v.emplace_back(beg, end);
            }
        }
        if (tabix) {
            const int32_t n_intv = c.i32();
            for (int32_t k = 0; k < n_intv; ++k) ref.linear.push_back(c.u64());
        }
    }
    return true;
}

BinIndex::Chunks BinIndex::query(size_t r, int64_t beg0, int64_t end0) const {
    Chunks out;
    if (r >= refs.size()) return out;
    const Ref &ref = refs[r];
    if (beg0 < 0) beg0 = 0;
    if (end0 <= beg0) end0 = beg0 + 1;
    const int64_t e = end0 - 1;
    uint64_t min_off = 0;  // the linear index, where one was loaded: nothing before it can overlap
    if (!ref.linear.empty()) min_off = ref.linear[std::min((size_t)(beg0 >> min_shift), ref.linear.size() - 1)];
    int s = min_shift + depth * 3;
    uint64_t t = 0;
    for (int l = 0; l <= depth; ++l) {
        uint64_t b0 = t + (uint64_t)(beg0 >> s), b1 = t + (uint64_t)(e >> s);
        // tabix: level 0 is bin 0 alone, whatever the position (the shift gives 0 only below 2^29)
        if (tabix && l == 0) b0 = b1 = 0;
        for (uint64_t b = b0; b <= b1; ++b) {
            const auto bi = ref.bins.find((uint32_t)b);
            if (bi == ref.bins.end()) continue;
            for (const auto &c : bi->second)
                if (c.second > min_off) out.emplace_back(std::max(c.first, min_off), c.second);  // (an end of 0: empty)
        }
        t += 1ull << (l * 3);
        s -= 3;
    }
    std::sort(out.begin(), out.end());
    return out;
}

}  // namespace nimpress
