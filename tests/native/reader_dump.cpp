// Test driver that pins what the genotype file readers hand out (no GPU, no libnps call: nimpress_host.hpp only, links
// the reader units of nimpress_amd/build.py's HOST_READER_SOURCES).
//   reader_dump <score file> <format>:<mode>:<path> [...]
// <format>: "-" (NIMPRESS_FORMAT unset), "DS" or "PL" (set before the open).  <mode>: scan = VCF::open(path); keep =
// VCF::open(path, &entries) with the score file's rows; stream1 / stream2 = openStreaming + fetch in windows of 1 / 2 rows.
// Per argument: a "== <argument>" line, the sample names, then "refused: <the reader's message>", or one line per record
// with every field of Variant (byte vectors as hex, FORMAT/DS values as float32 bit patterns).  The status is 0 whatever
// the files hold.  Its whole output is compared with tests/reader_dump_expected.txt by tests/test_reader_dump.py, which
// also builds it with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

#include "../../nimpress_amd/csrc/host/nimpress_host.hpp"

using namespace nimpress;

static void hex(std::string &out, const void *p, size_t n) {
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < n; ++i) {
        out += "0123456789abcdef"[b[i] >> 4];
        out += "0123456789abcdef"[b[i] & 15];
    }
}

static std::string recordLine(const Variant &v) {
    std::string s = "rec contig=" + v.contig + " pos=" + std::to_string(v.pos) + " id=" + v.id + " ref=" + v.ref + " alt=";
    for (size_t k = 0; k < v.alt.size(); ++k) s += (k ? "," : "") + v.alt[k];
    s += " filter=" + v.filter + " ploidy=" + std::to_string(v.ploidy) + " has_gt=" + std::to_string((int)v.has_gt) +
         " has_ds=" + std::to_string((int)v.has_ds) + " has_pl=" + std::to_string((int)v.has_pl) +
         " gt_bytes=" + std::to_string(v.gt_bytes) + " is_bed=" + std::to_string((int)v.is_bed) +
         " is_pgen=" + std::to_string((int)v.is_pgen) + " gts=";
    hex(s, v.gts.data(), v.gts.size() * sizeof(int32_t));
    s += " gt_raw=";
    hex(s, v.gt_raw.data(), v.gt_raw.size());
    s += " ds_per_sample=" + std::to_string(v.ds_per_sample) + " ds=";
    for (size_t k = 0; k < v.ds.size(); ++k) {
        uint32_t u;
        memcpy(&u, &v.ds[k], 4);
        char buf[16];
        snprintf(buf, sizeof buf, "%s%08x", k ? "," : "", u);
        s += buf;
    }
    s += " pl_per_sample=" + std::to_string(v.pl_per_sample) + " pl_bytes=" + std::to_string(v.pl_bytes) + " pl_raw=";
    hex(s, v.pl_raw.data(), v.pl_raw.size());
    return s;
}

static void dumpOne(const std::string &mode, const std::string &path, const ScoreFile &sf) {
    VCF vcf;
    std::vector<std::string> lines;
    try {
        if (mode == "scan" || mode == "keep") {
            if (!vcf.open(path, mode == "keep" ? &sf.entries : nullptr)) lines.push_back("not opened");
            for (const Variant &v : vcf.records) lines.push_back(recordLine(v));
        } else {
            const size_t window = mode == "stream2" ? 2 : 1;
            if (!vcf.openStreaming(path)) lines.push_back("no index");
            for (size_t a = 0; vcf.streaming && a < sf.entries.size(); a += window) {
                const size_t n = std::min(window, sf.entries.size() - a);
                lines.push_back("window " + std::to_string(a) + "+" + std::to_string(n));
                for (const Variant &v : vcf.fetch(sf.entries.data() + a, n)) lines.push_back(recordLine(v));
            }
        }
    } catch (const std::exception &e) {  // a file the readers refuse: a message, never a crash
        lines.push_back(std::string("refused: ") + e.what());
    }
    std::string names = "samples:";
    for (const std::string &s : vcf.samples) names += " [" + s + "]";
    puts(names.c_str());
    for (const std::string &l : lines) puts(l.c_str());
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    ScoreFile sf;
    if (!sf.open(argv[1])) return 3;
    for (int k = 2; k < argc; ++k) {
        const std::string arg = argv[k];
        const size_t c1 = arg.find(':'), c2 = c1 == std::string::npos ? c1 : arg.find(':', c1 + 1);
        if (c2 == std::string::npos) return 2;
        const std::string format = arg.substr(0, c1), mode = arg.substr(c1 + 1, c2 - c1 - 1), path = arg.substr(c2 + 1);
        if (mode != "scan" && mode != "keep" && mode != "stream1" && mode != "stream2") return 2;
        if (format == "-")
            unsetenv("NIMPRESS_FORMAT");
        else
            setenv("NIMPRESS_FORMAT", format.c_str(), 1);
        printf("== %s\n", arg.c_str());
        dumpOne(mode, path, sf);
    }
    return 0;
}
