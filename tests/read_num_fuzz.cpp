// read_num_fuzz.cpp -- the number parser of csrc/wt_read.h (wtr_number) against glibc's strtod, bit for bit (test infrastructure
// of tests/test_read_num_host.py; a stand-alone program, built with -fsanitize=address,undefined).  The header is included as
// plain C++ (-DWT_EMU: the emulator's form of the same text).  Numerals: every digit count 1 .. 20, the point at every place,
// exponents -30 .. 30 in every spelling, W = 2^53 and its neighbours, fractions with trailing zeros, what "%f" prints of random
// doubles.  Every numeral the parser takes as exact must be strtod's bits; every numeral it calls slow must truly lie outside
// the exact set (W above 2^53 or |E| above 22, decided here on the digits themselves).
#define WT_EMU 1
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

#include "../wiggletools_amd/csrc/wt_read.h"

static long long g_exact = 0, g_slow = 0;

// W above 2^53 or |E| above 22, from the digits: the definition, written a second time and differently
static bool outside(const std::string &s) {
    size_t i = s[0] == '-' ? 1 : 0;
    std::string ip, fp;
    for (; i < s.size() && s[i] >= '0' && s[i] <= '9'; i++) ip += s[i];
    if (i < s.size() && s[i] == '.') for (i++; i < s.size() && s[i] >= '0' && s[i] <= '9'; i++) fp += s[i];
    long ex = 0;
    if (i < s.size()) ex = strtol(s.c_str() + i + 1, nullptr, 10);
    while (!fp.empty() && fp.back() == '0') fp.pop_back();
    std::string d = ip + fp;
    d.erase(0, d.find_first_not_of('0'));
    if (d.empty()) return false;
    const long E = ex - (long) fp.size();
    const std::string lim = "9007199254740992";
    const bool big = d.size() > lim.size() || (d.size() == lim.size() && d > lim);
    return big || E < -22 || E > 22;
}

static bool check(const std::string &s) {
    WtrCtx c;
    c.text = (const unsigned char *) s.data(); c.n = (long long) s.size(); c.lo = 0; c.hi = 0; c.win = c.text; c.shift = 0;
    wtr_u64 bits = 0;
    int slow = 0;
    if (!wtr_number(c, 0, (long long) s.size(), &bits, &slow)) { printf("FAIL not a number: '%s'\n", s.c_str()); return false; }
    if (slow != (outside(s) ? 1 : 0)) { printf("FAIL slow %d: '%s'\n", slow, s.c_str()); return false; }
    if (slow) { g_slow++; return true; }
    const double v = strtod(s.c_str(), nullptr);
    uint64_t want;
    memcpy(&want, &v, 8);
    g_exact++;
    if (want != bits) { printf("FAIL '%s': strtod %016llx, header %016llx\n", s.c_str(), (unsigned long long) want, (unsigned long long) bits); return false; }
    return true;
}

static bool both_signs(const std::string &s) { return check(s) && check("-" + s); }

int main() {
    std::mt19937_64 rng(20261021);
    bool ok = true;
    char buf[64];
    const char *spell[] = {"e%d", "E%d", "e%+d", "E%+03d"};
    for (int round = 0; round < 60 && ok; round++)
        for (int nd = 1; nd <= 20 && ok; nd++) {
            std::string digits;
            for (int i = 0; i < nd; i++) digits += (char) ('0' + rng() % 10);
            if (round % 4 == 1) for (int i = nd / 2; i < nd; i++) digits[i] = '0';               // trailing zeros
            if (round % 4 == 2) digits[0] = '0';                                             // a leading zero
            for (int cut = 0; cut <= nd && ok; cut++) {
                std::string m = digits.substr(0, cut);
                if (cut < nd) m += "." + digits.substr(cut);
                ok = ok && both_signs(m);
                for (int e = -30; e <= 30 && ok; e++) {
                    snprintf(buf, sizeof buf, spell[(e + 30 + round) % 4], e);
                    ok = ok && both_signs(m + buf);
                }
            }
        }
    // W around 2^53 under every exponent; the ends of the table
    for (long long d = -3; d <= 3 && ok; d++)
        for (int e = -30; e <= 30 && ok; e++) {
            snprintf(buf, sizeof buf, "%llde%d", 9007199254740992ll + d, e);
            ok = ok && both_signs(buf);
            snprintf(buf, sizeof buf, "%lld.000e%d", 9007199254740992ll + d, e);
            ok = ok && both_signs(buf);
            snprintf(buf, sizeof buf, "900719925474.%04llde%d", 992ll + d, e);
            ok = ok && both_signs(buf);
        }
    // what the writer prints: "%f" of random doubles below 2^53 (all exact), and "%.17g" (mostly slow)
    for (int i = 0; i < 1000000 && ok; i++) {
        const uint64_t e = 1023 - 40 + rng() % 92;
        const uint64_t b = (rng() & 0x800fffffffffffffull) | (e << 52);
        double v;
        memcpy(&v, &b, 8);
        snprintf(buf, sizeof buf, "%f", v);
        ok = ok && check(buf);
        if (i % 4 == 0) { snprintf(buf, sizeof buf, "%.17g", v); ok = ok && check(buf); }
        if (i % 4 == 1) { snprintf(buf, sizeof buf, "%.6g", v); ok = ok && check(buf); }
    }
    for (const char *s : {"0", "-0", "0.000000", "-0.000000", "0e999", ".0", "000", "1e22", "1e-22", "1e23", "1e-23", "9007199254740992e22", "9007199254740993"})
        ok = ok && check(s);
    if (!ok) return 1;
    printf("checked %lld exact numerals bit for bit, %lld slow numerals outside the exact set\nread-num-fuzz-ok\n", g_exact, g_slow);
    return 0;
}
