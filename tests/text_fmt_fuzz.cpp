// text_fmt_fuzz.cpp -- the integer "%lf" of csrc/wt_text.h (wtx_num, wtx_put_num) against glibc's snprintf("%f"), byte for
// byte (test infrastructure of tests/test_text_fmt_host.py; a stand-alone program, built with -fsanitize=address,undefined).
// The header is included as plain C++ (-DWT_EMU: the emulator's form of the same text).  Values: every tie of the sixth
// decimal there is -- N + j/128 for odd j, the only fractions whose 10^6-fold ends in .5 -- over small and large N; both
// neighbours of 10^k - 5e-7; powers of two and their neighbours from the smallest denormal to 2^64; 2^53 +- 1 ulp; the largest
// narrow value; zeros, infinities and NaNs of either sign; then 1.5 million random mantissas under exponents 2^-80 .. 2^63 and
// random bit patterns until a million of them were narrow.  Wide values (finite, 2^64 and more) must be reported as such.
#define WT_EMU 1
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "../wiggletools_amd/csrc/wt_text.h"

static long long g_checked = 0, g_wide = 0;

static double from_bits(uint64_t b) {
    double v;
    memcpy(&v, &b, 8);
    return v;
}

static bool check(double v) {
    char want[400], got[64];
    memset(got, 0x7e, sizeof got);
    const int nw = snprintf(want, sizeof want, "%f", v);
    const WtxNum n = wtx_num(v);
    const bool wide = v - v == 0.0 && fabs(v) >= 18446744073709551616.0;
    if (wide != (n.kind == WTX_WIDE)) { printf("FAIL wide: %a\n", v); return false; }
    if (wide) { g_wide++; return true; }
    const WtxOut o = {(unsigned char *) got, 0, 40, 0};
    const long long ng = wtx_put_num(o, 0, n);
    g_checked++;
    if (ng != nw || ng != (long long) wtx_num_len(n) || memcmp(want, got, (size_t) nw) != 0 || got[ng] != 0x7e) {
        got[ng < 63 ? ng : 63] = 0;
        printf("FAIL %a: snprintf '%s' (%d), header '%s' (%lld, counted %u)\n", v, want, nw, got, ng, wtx_num_len(n));
        return false;
    }
    return true;
}

static bool both_signs(double v) { return check(v) && check(-v); }

int main() {
    std::mt19937_64 rng(20261120);
    bool ok = true;
    // ties
    for (int j = 1; j < 128 && ok; j += 2) {
        ok = ok && both_signs(j / 128.0);
        for (int t = 0; t < 200 && ok; t++) {
            const double N = (double) (rng() >> (19 + rng() % 45));          // up to 2^45: N + j/128 is exact
            ok = ok && both_signs(N + j / 128.0) && both_signs((double) (t * 5) + j / 128.0);
        }
    }
    // neighbours of 10^k - 5e-7, of powers of ten and of powers of two
    for (int k = 0; k <= 19 && ok; k++) {
        const double p = pow(10.0, k), x = p - 5e-7;
        for (double y : {x, nextafter(x, 0.0), nextafter(x, 1e300), p, nextafter(p, 0.0), nextafter(p, 1e300), p - 1.0, p - 0.5})
            ok = ok && both_signs(y);
    }
    for (int e = -1074; e <= 64 && ok; e++) {
        const double p = ldexp(1.0, e);
        ok = ok && both_signs(p) && both_signs(nextafter(p, 0.0)) && both_signs(nextafter(p, 1e300)) && both_signs(p * 1.5) && both_signs(p * 1.999);
    }
    for (double y : {0.0, 9007199254740992.0, 9007199254740991.0, 9007199254740994.0, 18446744073709549568.0, 18446744073709551616.0, 1.7976931348623157e308,
                     0.0078125, 0.0234375, 9.9999995, 0.9999995, 1.0000005, 1e-9, 4.9999995e-7, 5e-7, 5.000001e-7, 1.5e-6, 2.5e-6, (double) INFINITY})
        ok = ok && both_signs(y);
    for (uint64_t b : {0x7ff8000000000000ull, 0xfff8000000000000ull, 0x7ff0000000000001ull, 0xfff0000000000001ull, 0x7fffffffffffffffull, 0xffffffffffffffffull})
        ok = ok && check(from_bits(b));
    // random mantissas where the digits are: 2^-80 .. 2^63
    for (int i = 0; i < 1500000 && ok; i++) {
        const uint64_t e = 1023 - 80 + rng() % 144;
        ok = check(from_bits((rng() & 0x800fffffffffffffull) | (e << 52)));
    }
    // random bit patterns
    const long long before = g_checked;
    while (ok && g_checked - before < 1000000) ok = check(from_bits(rng()));
    if (!ok) return 1;
    printf("checked %lld values byte for byte, %lld wide values recognised\ntext-fmt-fuzz-ok\n", g_checked, g_wide);
    return 0;
}
