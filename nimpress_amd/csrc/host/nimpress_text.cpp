// nimpress_text.cpp -- see nimpress_host.hpp.  The host's text and common parts: string helpers with Nim stdlib
// semantics, score and BED files, the binomial statistics of the AF-mismatch warnings, the log, the time breakdown.
// No genotype file is read here and no libnps symbol is referenced.
#include "nimpress_internal.hpp"

#include <cerrno>
#include <charconv>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <sstream>
#include <stdexcept>

namespace nimpress {

// ---- where the time goes --------------------------------------------------------------------------------
static thread_local Timings g_timings;  // (per calling thread, like the error string of the C hooks)
Timings &timings() { return g_timings; }
void timingsReset() { g_timings = Timings(); }
double nowSeconds() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ------------------------------------------------------------------------------------------
// small text helpers with Nim stdlib semantics
static std::string stripTrailing(std::string s) {  // strip(leading = false)
    while (!s.empty() && (s.back() == ' ' || (s.back() >= '\t' && s.back() <= '\r'))) s.pop_back();
    return s;
}

std::vector<std::string> splitChar(const std::string &s, char sep) {
    std::vector<std::string> out;
    size_t a = 0;
    while (true) {
        size_t b = s.find(sep, a);
        if (b == std::string::npos) {
            out.push_back(s.substr(a));
            break;
        }
        out.push_back(s.substr(a, b - a));
        a = b + 1;
    }
    return out;
}

// lines as Nim's readLine / lines iterator yields them: terminators LF, CRLF or CR removed; a final
// unterminated line is a line; a trailing terminator does not create an extra empty line
static std::vector<std::string> splitLines(const std::string &text) {
    std::vector<std::string> out;
    size_t a = 0;
    const size_t n = text.size();
    while (a < n) {
        size_t b = a;
        while (b < n && text[b] != '\n' && text[b] != '\r') ++b;
        out.push_back(text.substr(a, b - a));
        if (b < n && text[b] == '\r' && b + 1 < n && text[b + 1] == '\n') ++b;
        a = b + 1;
    }
    return out;
}

static double parseFloatNim(const std::string &s) {
    if (s.empty()) throw std::runtime_error("invalid float: (empty)");
    errno = 0;
    char *end = nullptr;
    const double v = strtod(s.c_str(), &end);
    if (end == s.c_str() || *end != 0) throw std::runtime_error("invalid float: " + s);
    return v;
}

int64_t parseIntNim(const std::string &s) {
    if (s.empty()) throw std::runtime_error("invalid integer: (empty)");
    size_t i = 0;
    if (s[0] == '+' || s[0] == '-') i = 1;
    if (i == s.size()) throw std::runtime_error("invalid integer: " + s);
    for (size_t k = i; k < s.size(); ++k)
        if (s[k] < '0' || s[k] > '9') throw std::runtime_error("invalid integer: " + s);
    return strtoll(s.c_str(), nullptr, 10);
}

bool readFile(const std::string &path, std::string &out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    std::ostringstream ss;
    ss << f.rdbuf();
    out = ss.str();
    return true;
}

// Nim's `$float` as the reference prints a score (nim:753): "%.16g", ".0" appended where the text has neither '.', 'e'
// nor 'n'.  std::to_chars(general, 16) is "%.16g" by definition (checked against snprintf on a million values) at a
// third of its cost; writes at most 32 characters, returns their number.
std::string formatFloat(double x) {
    char buf[32];
    return std::string(buf, formatFloatTo(x, buf));
}

// ------------------------------------------------------------------------------------------
bool parseEnum(const std::string &s, ImputeMethodLocus &out) {
    static const char *names[] = {"ps", "homref", "fail", "ignore"};
    for (int i = 0; i < 4; ++i)
        if (s == names[i]) {
            out = (ImputeMethodLocus)i;
            return true;
        }
    return false;
}
bool parseEnum(const std::string &s, ImputeMethodMissing &out) {
    static const char *names[] = {"homref", "ignore"};
    for (int i = 0; i < 2; ++i)
        if (s == names[i]) {
            out = (ImputeMethodMissing)i;
            return true;
        }
    return false;
}
bool parseEnum(const std::string &s, ImputeMethodSample &out) {
    static const char *names[] = {"ps", "homref", "fail", "int_ps", "int_fail"};
    for (int i = 0; i < 5; ++i)
        if (s == names[i]) {
            out = (ImputeMethodSample)i;
            return true;
        }
    return false;
}

// ------------------------------------------------------------------------------------------
// ScoreFile  nim:233-254
bool ScoreFile::open(const std::string &path) {
    std::string text;
    if (!readFile(path, text)) return false;
    const std::vector<std::string> lines = splitLines(text);
    if (lines.size() < 5) throw std::runtime_error("score file has fewer than 5 header lines: " + path);
    name = stripTrailing(lines[0]);
    desc = stripTrailing(lines[1]);
    cite = stripTrailing(lines[2]);
    genomever = stripTrailing(lines[3]);
    offset = parseFloatNim(stripTrailing(lines[4]));
    entries.clear();
    for (size_t i = 5; i < lines.size(); ++i) {
        const std::vector<std::string> parts = splitChar(stripTrailing(lines[i]), '\t');
        if (parts.size() != 6)  // doAssert lineparts.len == 6, nim:252
            throw std::runtime_error("score file " + path + " line " + std::to_string(i + 1) +
                                     ": expected 6 tab-separated fields");
        ScoreEntry e;
        e.contig = parts[0];
        e.pos = parseIntNim(parts[1]);
        e.refseq = parts[2];
        e.easeq = parts[3];
        e.beta = parseFloatNim(parts[4]);
        e.eaf = parseFloatNim(parts[5]);
        entries.push_back(std::move(e));
    }
    return true;
}

// ------------------------------------------------------------------------------------------
// GenomeIntervals  nim:278-345
bool loadBedIntervals(GenomeIntervals &ivals, const std::string &path) {
    std::string text;
    if (!readFile(path, text)) return false;
    ivals.init = false;
    ivals.contigIntervals.clear();
    for (const std::string &line : splitLines(text)) {
        const std::vector<std::string> parts = splitChar(stripTrailing(line), '\t');
        if (parts.size() < 3) throw std::runtime_error("BED line with fewer than 3 fields: " + line);
        ivals.contigIntervals[parts[0]].emplace_back(parseIntNim(parts[1]), parseIntNim(parts[2]));
    }
    ivals.init = true;
    return true;
}

bool isVariantCovered(const ScoreEntry &e, const GenomeIntervals &ivals, std::string *warning) {
    auto it = ivals.contigIntervals.find(e.contig);
    if (it == ivals.contigIntervals.end()) {  // nim:325-328
        if (warning) *warning = "Contig " + e.contig + " not present within the coverage BED file.";
        return false;
    }
    // the reference pre-selects overlapping intervals with lapper (nim:337); the decision is the
    // containment predicate of nim:310-311
    for (const auto &iv : it->second)
        if (iv.first < e.pos && iv.second >= e.stop()) return true;
    return false;
}

// ------------------------------------------------------------------------------------------
// stats for the AF-mismatch warnings  nim:50-188
static double lbinom(int64_t n, int64_t k) {
    return lgamma((double)n + 1.0) - lgamma((double)k + 1.0) - lgamma((double)(n - k) + 1.0);
}

double dbinom(int64_t x, int64_t n, double p) {
    if ((x == 0 && p == 0.0) || (x == n && p == 1.0)) return 1.0;
    return exp(lbinom(n, x) + (double)x * log(p) + (double)(n - x) * log(1.0 - p));
}

static double betacf(double a, double b, double x) {  // modified Lentz, 100 iterations, eps 3e-7
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0, tiny = 1.0e-30;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= 100; ++m) {
        const double mf = (double)m;
        double aa = mf * (b - mf) * x / ((qam + 2 * mf) * (a + 2 * mf));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + mf) * (qab + mf) * x / ((a + 2 * mf) * (qap + 2 * mf));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) < 3.0e-7) return h;
    }
    return std::numeric_limits<double>::quiet_NaN();  // not converged (nim:117)
}

double betai(double a, double b, double x) {
    if (!(x >= 0.0 && x <= 1.0)) throw std::runtime_error("betai: x outside [0,1]");
    if (a == 0.0 || b == 0.0) return std::numeric_limits<double>::infinity();
    if (x == 0.0) return 0.0;
    if (x == 1.0) return 1.0;
    const double bt = exp(lgamma(a + b) - lgamma(a) - lgamma(b) + a * log(x) + b * log(1.0 - x));
    if (x < (a + 1.0) / (a + b + 2.0)) return bt * betacf(a, b, x) / a;
    return 1.0 - bt * betacf(b, a, 1.0 - x) / b;
}

double pbinom(int64_t x, int64_t n, double p) {
    if (x < 0) return 0.0;
    if (x == n) return 1.0;
    return 1.0 - betai((double)x + 1.0, (double)(n - x), p);
}

double binomTest(int64_t x, int64_t n, double p) {
    if (p == 0.0) return x == 0 ? 1.0 : 0.0;
    if (p == 1.0) return x == n ? 1.0 : 0.0;
    const double probx = dbinom(x, n, p), expected = (double)n * p;
    if (fabs((double)x / expected - 1.0) < 1.0e-6) return 1.0;
    const double bound = probx * (1.0 + 1.0e-7);
    int64_t y = 0;
    if ((double)x < expected) {
        for (int64_t xi = (int64_t)ceil(expected); xi <= n; ++xi)
            if (dbinom(xi, n, p) <= bound) ++y;
        return pbinom(x, n, p) + (1.0 - pbinom(n - y, n, p));
    }
    for (int64_t xi = 0; xi <= (int64_t)floor(expected); ++xi)
        if (dbinom(xi, n, p) <= bound) ++y;
    return pbinom(y - 1, n, p) + (1.0 - pbinom(x - 1, n, p));
}

// The reference finds the far integration limit by enumerating up to n dbinom() values per call
// (nim:173-187: ~27 ms per score row at 500 000 samples, ten times the dosage arithmetic).  On the
// enumerated side of the mode dbinom is monotone, so the set {xi : dbinom(xi) <= probx*(1+1e-7)} is
// an interval ending at the boundary of the range and its size follows from a bisection:
// O(log n) dbinom evaluations, same count y, same p-value (tests/test_host_logic.py compares it with
// the literal enumeration on thousands of cases).
double binomTestFast(int64_t x, int64_t n, double p) {
    if (p == 0.0) return x == 0 ? 1.0 : 0.0;
    if (p == 1.0) return x == n ? 1.0 : 0.0;
    const double probx = dbinom(x, n, p), expected = (double)n * p;
    if (fabs((double)x / expected - 1.0) < 1.0e-6) return 1.0;
    const double bound = probx * (1.0 + 1.0e-7);
    if ((double)x < expected) {
        // xi in [lo, n], dbinom non-increasing: first xi with dbinom(xi) <= bound
        int64_t lo = (int64_t)ceil(expected), hi = n + 1;  // answer in [lo, n+1]
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (dbinom(mid, n, p) <= bound)
                hi = mid;
            else
                lo = mid + 1;
        }
        const int64_t y = n - lo + 1;
        return pbinom(x, n, p) + (1.0 - pbinom(n - y, n, p));
    }
    // xi in [0, top], dbinom non-decreasing: last xi with dbinom(xi) <= bound
    int64_t lo = -1, hi = (int64_t)floor(expected);  // answer in [-1, top]
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (dbinom(mid, n, p) <= bound)
            lo = mid;
        else
            hi = mid - 1;
    }
    const int64_t y = lo + 1;
    return pbinom(y - 1, n, p) + (1.0 - pbinom(x - 1, n, p));
}

// ------------------------------------------------------------------------------------------
void Log::warn(const std::string &m) {
    lines.push_back("WARN " + m);
    if (echo) {
        fputs(lines.back().c_str(), stdout);
        fputc('\n', stdout);
    }
}
void Log::fatal(const std::string &m) {
    lines.push_back("FATAL " + m);
    if (echo) {
        fputs(lines.back().c_str(), stdout);
        fputc('\n', stdout);
    }
}

}  // namespace nimpress
