// isearch_fuzz.cpp -- stand-alone host program of tests/test_isearch_host.py: the window index's lane search
// (csrc/wt_isearch.h) against std::lower_bound, with every read of finish[] counted.  Built with
// -fsanitize=address,undefined and run as a binary.  Prints "mean reads: baseline X interpolation Y" and
// "isearch-fuzz-ok" when every assertion held; exits 1 at the first one that did not.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../include/wiggletools_amd.h"
#include "../wiggletools_amd/csrc/wt_isearch.h"

static long long g_reads = 0;

// finish[] of one bracket's track behind a counter; a read outside [0, n) is a failure of its own
struct CountFin {
    const int32_t *p;
    long long n;
    long long operator()(long long x) const {
        if (x < 0 || x >= n) { printf("FAIL: read of entry %lld outside [0, %lld)\n", x, n); exit(1); }
        g_reads++;
        return (long long) p[x];
    }
    long long operator[](long long x) const { return (*this)(x); }
};

// The routine this change replaces (csrc/wt_core.h wt_lane_lower_bound before the interpolation steps), verbatim but for the
// type of `fin`: the baseline of the read counts.
static long long baseline_lower_bound(const CountFin &fin, long long lo, long long hi, long long g, long long b) {
    if (lo >= hi) return lo;
    if ((long long) fin[g] >= b) {
        hi = g;
        for (long long d = 1;; d <<= 1) {
            const long long q = hi - d;
            if (q < lo) break;
            if ((long long) fin[q] < b) { lo = q + 1; break; }
            hi = q;
        }
    } else {
        lo = g + 1;
        for (long long d = 1;; d <<= 1) {
            const long long q = lo + d - 1;
            if (q >= hi) break;
            if ((long long) fin[q] >= b) { hi = q; break; }
            lo = q + 1;
        }
    }
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if ((long long) fin[mid] < b) lo = mid + 1; else hi = mid;
    }
    return lo;
}

static int ceil_log2(long long n) {
    int k = 0;
    while (((long long) 1 << k) < n) k++;
    return k;
}

static long long g_cases = 0, g_max_reads = 0;

// one search of [lo, hi) of v for b from guess g with `density`: equality with std::lower_bound and the read bound
static void check(const std::vector<int32_t> &v, long long lo, long long hi, long long g, long long b, float density, const char *what) {
    const long long want = std::lower_bound(v.begin() + lo, v.begin() + hi, b, [](int32_t x, long long y) { return (long long) x < y; }) - v.begin();
    const CountFin fin{v.data(), (long long) v.size()};
    g_reads = 0;
    const long long got = wt_interp_lower_bound(fin, lo, hi, g, b, density);
    const long long reads = g_reads, n = hi - lo;
    const long long bound = 2 * ceil_log2(n) + 6;
    g_cases++;
    if (reads > g_max_reads) g_max_reads = reads;
    if (got != want) { printf("FAIL %s: [%lld, %lld) g %lld b %lld density %g: got %lld, lower_bound %lld\n", what, lo, hi, g, b, (double) density, got, want); exit(1); }
    if (reads > bound) { printf("FAIL %s: [%lld, %lld) g %lld b %lld density %g: %lld reads above the bound %lld\n", what, lo, hi, g, b, (double) density, reads, bound); exit(1); }
    // the plain routine through the same door (what the coarse rows of the patch kernels call)
    g_reads = 0;
    const long long got0 = wt_gallop_lower_bound(fin, lo, hi, g, b);
    if (got0 != want || g_reads > bound) { printf("FAIL %s (gallop): [%lld, %lld) g %lld b %lld: got %lld, lower_bound %lld, %lld reads\n", what, lo, hi, g, b, got0, want, g_reads); exit(1); }
}

// every boundary, guess and density worth trying on the bracket [lo, hi) of v
static void sweep(const std::vector<int32_t> &v, long long lo, long long hi, std::mt19937_64 &rng, const char *what) {
    const long long n = hi - lo;
    std::vector<long long> bs;
    if (n > 0) {
        const long long first = v[lo], last = v[hi - 1];
        for (long long d : {-70000ll, -2ll, -1ll, 0ll, 1ll}) bs.push_back(first + d);              // below and at the first entry
        for (long long d : {-1ll, 0ll, 1ll, 2ll, 70000ll}) bs.push_back(last + d);                 // at and above the last
        bs.push_back(0); bs.push_back(-5); bs.push_back((long long) WTAMD_MAX_COORD); bs.push_back((long long) WTAMD_MAX_COORD + 65536);
        const int samples = n <= 64 ? (int) n : 48;
        for (int k = 0; k < samples; k++) {
            const long long x = n <= 64 ? lo + k : lo + (long long) (rng() % (uint64_t) n);
            for (long long d : {-1ll, 0ll, 1ll}) bs.push_back((long long) v[x] + d);               // an entry, one below, one above
        }
        for (int k = 0; k < 16; k++) bs.push_back(first + (long long) (rng() % (uint64_t) (last - first + 1)));
    } else {
        bs.push_back(0); bs.push_back(12345);
    }
    float true_density = 0.0f;
    if (n > 1 && v[hi - 1] > v[lo]) true_density = (float) n / (float) ((long long) v[hi - 1] - v[lo]);
    const float densities[] = {true_density, 0.0f, -1.0f, 1e-9f, 1.0f / 16, 1.0f, 1e9f, 3e38f};
    for (long long b : bs) {
        std::vector<long long> gs;
        if (n > 0) {
            gs.push_back(lo); gs.push_back(hi - 1); gs.push_back(lo + n / 2);
            gs.push_back(lo + (long long) (rng() % (uint64_t) n));
            long long gi = lo + (long long) ((double) (b - v[lo]) * true_density);       // where a caller that interpolates would start
            gs.push_back(std::min(std::max(gi, lo), hi - 1));
        } else {
            gs.push_back(lo);
        }
        for (long long g : gs)
            for (float d : densities) check(v, lo, hi, g, b, d, what);
    }
}

static std::vector<int32_t> bench_like(long long n, int32_t base, std::mt19937_64 &rng) {
    // contiguous runs of 1 + Geometric(1/16) base pairs from `base`: finish[] is their running sum
    std::geometric_distribution<int> geo(1.0 / 16);
    std::vector<int32_t> v((size_t) n);
    long long pos = base;
    for (long long k = 0; k < n; k++) { pos += 1 + geo(rng); v[(size_t) k] = (int32_t) pos; }
    return v;
}

int main() {
    std::mt19937_64 rng(20240607);
    const long long sizes[] = {0, 1, 2, 3, 4, 5, 7, 8, 9, 17, 63, 64, 65, 1000, 4097, 32768, 40000};
    for (long long n : sizes) {
        // (a few entries around the bracket: a search that leaves it reads them and gets another answer, or trips the counter's bounds)
        const long long pad = 3, tot = n + 2 * pad;
        {   // the bench's distribution
            std::vector<int32_t> v = bench_like(tot, 1000, rng);
            sweep(v, pad, pad + n, rng, "bench");
            sweep(v, 0, tot, rng, "bench, whole array");
        }
        {   // all entries equal
            std::vector<int32_t> v((size_t) tot, 777777);
            sweep(v, pad, pad + n, rng, "equal");
        }
        {   // 99 % of the runs in the first 1 % of the coordinates, then one far run
            std::vector<int32_t> v = bench_like(tot, 5, rng);
            const long long last_near = v[(size_t) tot - 2];
            v[(size_t) tot - 1] = (int32_t) std::min<long long>(last_near * 100 + 100, WTAMD_MAX_COORD);
            sweep(v, 0, tot, rng, "clustered");
            if (n > 0) sweep(v, pad, tot, rng, "clustered, inner bracket");
        }
        {   // coordinates up to WTAMD_MAX_COORD: a far first entry, a dense end
            std::vector<int32_t> v = bench_like(tot, 0, rng);
            const long long shift = (long long) WTAMD_MAX_COORD - v[(size_t) tot - 1];
            for (auto &x : v) x = (int32_t) (x + shift);
            if (tot > 1) v[0] = 1;
            sweep(v, 0, tot, rng, "near the maximum coordinate");
            sweep(v, pad, pad + n, rng, "near the maximum coordinate, inner bracket");
        }
        {   // two entries as far apart as coordinates go, the bracket between them
            std::vector<int32_t> v((size_t) tot, 1);
            for (long long k = tot / 2; k < tot; k++) v[(size_t) k] = WTAMD_MAX_COORD;
            sweep(v, 0, tot, rng, "step");
        }
    }

    // The bench's shape: a wave's 64 boundaries over a bracket of (about) 32 768 runs, every lane from its linear guess between
    // the two coarse answers, as wt_index_search_kernel searches.  Mean reads of the baseline and of the interpolation search.
    const int strips = 48;
    const long long per_strip = 32768;
    std::vector<int32_t> v = bench_like(per_strip * (strips + 1), 1, rng);
    const long long first = v.front(), last = v.back();
    const long long W = (last - first) / ((long long) (strips + 1) * 64);       // (window width: 64 windows hold 32 768 runs on average)
    const CountFin fin{v.data(), (long long) v.size()};
    auto lb = [&](long long b) { return (long long) (std::lower_bound(v.begin(), v.end(), b, [](int32_t x, long long y) { return (long long) x < y; }) - v.begin()); };
    long long reads_base = 0, reads_new = 0, searches = 0;
    for (int s = 0; s < strips; s++) {
        const long long bA = first + (long long) s * 64 * W, bB = bA + 64 * W;
        const long long A = lb(bA), B = lb(bB);
        const float density = (float) (B - A) / (float) (bB - bA);
        for (int lane = 0; lane < 64; lane++) {
            const long long b = bA + lane * W;
            long long g = A + (((B - A) * lane) >> 6);
            if (g > B - 1) g = B - 1;
            const long long want = lb(b);
            g_reads = 0;
            const long long r0 = baseline_lower_bound(fin, A, B, g, b);
            reads_base += g_reads;
            g_reads = 0;
            const long long r1 = wt_interp_lower_bound(fin, A, B, g, b, density);
            reads_new += g_reads;
            if (g_reads > 2 * ceil_log2(B - A) + 6) { printf("FAIL bench shape: %lld reads\n", g_reads); return 1; }
            if (r0 != want || r1 != want) { printf("FAIL bench shape: strip %d lane %d: baseline %lld interpolation %lld lower_bound %lld\n", s, lane, r0, r1, want); return 1; }
            searches++;
        }
    }
    const double mean_base = (double) reads_base / (double) searches, mean_new = (double) reads_new / (double) searches;
    printf("checked %lld searches, most reads in one %lld\n", g_cases, g_max_reads);
    printf("mean reads: baseline %.3f interpolation %.3f (%lld searches, 64 boundaries per bracket of %lld runs)\n", mean_base, mean_new, searches, per_strip);
    if (!(mean_new < mean_base)) { printf("FAIL: the interpolation search reads no less than the baseline\n"); return 1; }
    printf("isearch-fuzz-ok\n");
    return 0;
}
