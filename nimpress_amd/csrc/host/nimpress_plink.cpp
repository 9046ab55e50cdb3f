// nimpress_plink.cpp -- see nimpress_readers.hpp.  The PLINK filesets: PLINK 1 .bed + .bim + .fam and the one PLINK 2
// flavour that is read, .pgen storage mode 0x02 (fixed-width hard calls) + .pvar + .psam.
#include "nimpress_readers.hpp"

#include <algorithm>

namespace nimpress {

bool openPlinkFileset(const std::string &path, const RegionMap *wanted, std::vector<std::string> &samples,
                      std::vector<Variant> &records) {
    FILE *f = fopen(path.c_str(), "rb");
    unsigned char magic[3] = {0, 0, 0};
    const bool is_bed = f && fread(magic, 1, 3, f) == 3 && magic[0] == 0x6c && magic[1] == 0x1b;
    if (!is_bed) {
        if (f) fclose(f);
        return false;
    }
    struct Closer {
        FILE *f;
        ~Closer() { fclose(f); }
    } closer{f};
    // byte 3 = storage mode: 0x01 PLINK 1 .bed (variant-major), 0x02 PLINK 2 .pgen with fixed-width hard-call
    // records (12-byte header: magic, mode, uint32 variants, uint32 samples, one flag byte; then
    // ceil(N/4) bytes per variant, the 2-bit code = number of ALT alleles, 3 = missing).  Nothing else of
    // the .pgen family is read (variable-width records, dosages, multi-allelic hard calls).
    // PARITY UNPINNED: neither plink2 nor the format's specification is in this image; the layout is written
    // from the published description and pinned only by the build's own writer (tests/pgenwriter.py).
    const bool pgen = magic[2] == 2;
    if (magic[2] == 0) throw std::runtime_error("sample-major .bed files are not supported");
    if (magic[2] != 1 && !pgen)
        throw std::runtime_error("PLINK 2 .pgen storage mode 0x" + std::string(1, "0123456789abcdef"[magic[2] >> 4]) +
                                 std::string(1, "0123456789abcdef"[magic[2] & 15]) +
                                 " is not supported (only 0x02: fixed-width hard calls; plink2 --make-pgen fixed-width, "
                                 "or convert with --make-bed)");
    std::string prefix = path;
    if (prefix.size() > 4 && (prefix.compare(prefix.size() - 4, 4, ".bed") == 0)) prefix.resize(prefix.size() - 4);
    if (prefix.size() > 5 && (prefix.compare(prefix.size() - 5, 5, ".pgen") == 0)) prefix.resize(prefix.size() - 5);
    std::string fam, bim;
    bool pvar = false, psam = false;
    if (pgen) {  // .pvar / .psam, or the PLINK 1 .bim / .fam next to the .pgen
        pvar = readFile(prefix + ".pvar", bim);
        psam = readFile(prefix + ".psam", fam);
        if ((!pvar && !readFile(prefix + ".bim", bim)) || (!psam && !readFile(prefix + ".fam", fam)))
            throw std::runtime_error("cannot open " + prefix + ".pvar / .psam (or .bim / .fam) next to the .pgen file");
    } else if (!readFile(prefix + ".fam", fam) || !readFile(prefix + ".bim", bim)) {
        throw std::runtime_error("cannot open " + prefix + ".fam / .bim next to the .bed file");
    }
    size_t header_bytes = 3;
    uint32_t pgen_m = 0, pgen_n = 0;
    if (pgen) {
        unsigned char h[9];
        if (fread(h, 1, 9, f) != 9) throw std::runtime_error("truncated .pgen header");
        memcpy(&pgen_m, h, 4);
        memcpy(&pgen_n, h + 4, 4);
        header_bytes = 12;
    }
    auto fields = [](const std::string &line) {
        std::vector<std::string> out;
        size_t i = 0;
        while (i < line.size()) {
            while (i < line.size() && (line[i] == ' ' || line[i] == '\t' || line[i] == '\r')) ++i;
            size_t j = i;
            while (j < line.size() && line[j] != ' ' && line[j] != '\t' && line[j] != '\r') ++j;
            if (j > i) out.push_back(line.substr(i, j - i));
            i = j;
        }
        return out;
    };
    size_t iid_col = 1;  // .fam: FID IID ...; .psam: the column its header line calls IID
    for (const std::string &ln : splitChar(fam, '\n')) {
        const std::vector<std::string> c = fields(ln);
        if (c.empty()) continue;
        if (psam && c[0][0] == '#') {
            if (c[0] == "#IID") iid_col = 0;
            else if (c[0] == "#FID") iid_col = 1;
            else continue;  // other comment lines
            if (iid_col >= c.size() || (iid_col == 1 && c[1] != "IID")) throw std::runtime_error("bad .psam header line");
            continue;
        }
        if (c.size() <= iid_col) throw std::runtime_error(psam ? "bad .psam line" : "bad .fam line");
        samples.push_back(c[iid_col]);  // IID
    }
    if (pgen && pgen_n != samples.size())
        throw std::runtime_error(".pgen header says " + std::to_string(pgen_n) + " samples, the sample file lists " +
                                 std::to_string(samples.size()));
    const size_t row_bytes = (samples.size() + 3) / 4;
    size_t row = 0;
    // .pvar: '##' meta lines, then '#CHROM POS ID REF ALT ...' naming the columns; without that line the file
    // has the .bim layout (chrom, id, cM, pos, ALT = A1, REF = A2)
    int col_chrom = 0, col_id = 1, col_pos = 3, col_alt = 4, col_ref = 5;
    size_t min_cols = 6;
    for (const std::string &ln : splitChar(bim, '\n')) {
        const std::vector<std::string> c = fields(ln);
        if (c.empty()) continue;
        if (pvar && c[0].size() >= 2 && c[0][0] == '#' && c[0][1] == '#') continue;
        if (pvar && c[0][0] == '#' && c[0] != "#CHROM") continue;  // (any other comment line: not a record)
        if (pvar && c[0] == "#CHROM") {
            col_chrom = 0;
            col_id = col_pos = col_alt = col_ref = -1;
            for (size_t k = 1; k < c.size(); ++k) {
                if (c[k] == "POS") col_pos = (int)k;
                if (c[k] == "ID") col_id = (int)k;
                if (c[k] == "REF") col_ref = (int)k;
                if (c[k] == "ALT") col_alt = (int)k;
            }
            if (col_pos < 0 || col_ref < 0 || col_alt < 0) throw std::runtime_error(".pvar header line lacks POS / REF / ALT");
            min_cols = (size_t)std::max(std::max(col_pos, col_ref), std::max(col_alt, col_id)) + 1;
            continue;
        }
        if (c.size() < min_cols) throw std::runtime_error(pgen ? "bad .pvar / .bim line" : "bad .bim line");
        Variant v;
        v.contig = c[(size_t)col_chrom];
        v.id = col_id >= 0 ? c[(size_t)col_id] : ".";
        v.pos = parseIntNim(c[(size_t)col_pos]);
        v.ref = c[(size_t)col_ref];           // .bed: A2; .pgen: REF
        v.alt.push_back(c[(size_t)col_alt]);  // .bed: A1; .pgen: ALT
        if (pgen && v.alt[0].find(',') != std::string::npos)
            throw std::runtime_error("multi-allelic .pvar record at " + v.contig + ":" + std::to_string(v.pos) +
                                     ": not representable in fixed-width hard-call records");
        v.filter = ".";
        v.is_bed = !pgen;
        v.is_pgen = pgen;
        v.gt_bytes = 0;
        v.ploidy = 2;
        const int64_t len = (int64_t)std::max(v.ref.size(), v.alt[0].size());
        if (!wanted || overlapsWanted(*wanted, v.contig, v.pos, v.pos + len - 1)) {
            v.gt_raw.resize(row_bytes);
            if (row_bytes &&
                (fseeko(f, (off_t)(header_bytes + row * row_bytes), SEEK_SET) != 0 ||
                 fread(v.gt_raw.data(), 1, row_bytes, f) != row_bytes))
                throw std::runtime_error(pgen ? "truncated .pgen file" : "truncated .bed file");
            records.push_back(std::move(v));
        }
        ++row;
    }
    if (pgen) {
        // the records are mapped to rows by line index alone: a .pvar that does not belong to this .pgen would be
        // scored with another variant's genotypes, silently.  The header's variant count and the file's length
        // must both agree with what was read.
        if (row != pgen_m)
            throw std::runtime_error(".pgen header says " + std::to_string(pgen_m) + " variants, " + prefix +
                                     (pvar ? ".pvar" : ".bim") + " lists " + std::to_string(row));
        if (fseeko(f, 0, SEEK_END) != 0) throw std::runtime_error("cannot seek in the .pgen file");
        const off_t size = ftello(f);
        if ((uint64_t)size != (uint64_t)header_bytes + (uint64_t)pgen_m * row_bytes)
            throw std::runtime_error(".pgen file is " + std::to_string((long long)size) + " bytes, " +
                                     std::to_string(pgen_m) + " fixed-width records of " + std::to_string(samples.size()) +
                                     " samples are " + std::to_string((unsigned long long)header_bytes + (unsigned long long)pgen_m * row_bytes));
    }
    return true;
}

}  // namespace nimpress
