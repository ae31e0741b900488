// wt_profile.h -- region profiles over whole run lists (device + -DWT_EMU): what the reference's ProfileMultiplexer
// (src/apply.c:355-366; the parser's `profile` / `profiles`, commandParser.c:862-905) computes through regionProfile
// (src/plots.c:27-64): the dataset under every region squeezed or stretched onto `width` bins.  This header is the single
// source of the logic.  It is compiled
//   * by hipcc for gfx950 inside csrc/wt_profile.hip (the product), and
//   * by g++ with -DWT_EMU inside tests/profile_emu.cpp, which runs the workgroups of every pass one after the other in any
//     order on the CPU.
// It is written in the manner of csrc/wt_apply.h and reuses its argument block, its validation and, through it, the staged
// window search of csrc/wt_region.h.
//
// Input: exactly that of wt_apply.h -- a dataset D and regions R with the same number of segments; D sorted, start < finish
// and DISJOINT; R sorted by start, free to overlap, nest or repeat; no negative start; fewer than 2^31 runs -- and width >= 1.
//
// The reference's rule.  Region [rs, rf), L = rf - rs, W = width, c = W / (double) L, r(i) = (int) round((double) i * c) with
// C's round, positions relative to rs.  The reference serves regionProfile
//   * one run [i, i + 1) with the dataset's value for every covered position i, and
//   * ONE run [a, b) with the default value for every maximal uncovered stretch.
// A run [a, b) with value v that is not NaN has start = r(a), finish = r(b), finish <= start -> start + 1, finish > W -> W,
// and gives v / (finish - start) to every bin of [start, finish).
//
// The closed form the passes use.  r is monotone, so with b_j = the smallest i in [0, L] with r(i) >= j (L + 1 without one):
//   * the positions of bin j are [b_j, b_{j+1}) when that is not empty, each with its value / 1 -- except the last one, whose
//     range may reach further (divisor n = min(max(r(i + 1), r(i) + 1), W) - r(i), computed, not assumed);
//   * when it is empty (c > 1: a position stretches over several bins) the one contributor is position b_j - 1;
//   * a gap [a, b) touches bin j iff a < b_{j+1} and (b >= b_{j+1} or a >= b_j).
// Consequences that are the reference's, not departures: bin 0 collects about half as many positions as the others; with
// L >= 2 W the last positions have r(i) == W and are dropped; an uncovered stretch counts as ONE sample of the default however
// long it is.  b_j comes from the estimate ceil((j - 0.5) / c), corrected by evaluating r itself on the neighbours.
//
// Arithmetic: a bin's terms are added in position order, a run piece of len positions as len * v (the last position of the
// bin's range apart, as v / n).  A bin with at most WPR_SMALL runs under it is summed by one lane in order; a larger one by
// WPR_WAVE lanes that take contiguous shares of its runs in order and merge pairwise, lower share first.  A region's row is a
// function of the region, its dataset segment, the default and W alone.
//
// Departures, as in wt_apply.h: the default is the double given (the reference truncates it to float, apply.c:42); every
// region sees its dataset whole (the reference seeks to the finish of the last region of a buffered group, apply.c:311).
//
// Passes (no pass waits for another workgroup, no atomics on the results):
//   valid   wap_valid_block, either side
//   bounds  a tile of WAP_TILE regions stages its dataset window (wrg_window); every region stores {lo, hi - lo}
//   then per BATCH of regions (a power of two, at most WPR_BATCH_DOUBLES / W of them, at least one):
//   bins    one lane per (region, bin): b_j, b_{j+1}, two binary searches inside [lo, hi); LANE REGIME: the lane finishes the
//           bin.  WAVE REGIME: it only sets its bit in the workgroup's mask; the workgroup stores the mask and its count.
//   scan    of the counts (wcv_scan_block)
//   heavy   one wavefront per wave-regime bin (four per workgroup), found by binary search over the scanned counts and the
//           mask: 64 contiguous shares, merged pairwise through LDS
//   and in SUM mode (WPR_SUM: column sums of all rows):
//   fold    rows i and i + s of the batch, i a multiple of 2 s, are added (lower first) for s = 1, 2, 4, ... three levels a
//           launch; a row without a partner is carried unchanged.  Batches are aligned, so the batch sums are nodes of ONE
//           tree over the call's region index, and a binary counter of rows (add) merges them by the same rule: the sum has
//           the same bits whatever the batch size.
//
// Scratch: 16 bytes per region + per batch 40 bytes per 256 bins of the batch; in SUM mode also 8 bytes x (bins of a batch
// + W x (2 + log2 of the number of batches)).  A batch holds at most max(W, WPR_BATCH_DOUBLES) bins: 32 MiB of rows.
#ifndef WT_PROFILE_H_
#define WT_PROFILE_H_

#include <math.h>

#include "wt_apply.h"

#define WPR_BLOCK WAP_BLOCK
#define WPR_SMALL 32                            // runs under a bin its own lane finishes
#define WPR_WAVE 64                             // shares of a wave-regime bin
#define WPR_WAVES (WPR_BLOCK / WPR_WAVE)
#define WPR_FOLD 8                              // rows one lane of the fold pass merges: three levels
#define WPR_BATCH_DOUBLES (1ll << 22)           // bins of a batch

#define WPR_SUM 1u

enum { WPR_K_VALID_D = 0, WPR_K_VALID_R, WPR_K_BOUNDS, WPR_K_BINS, WPR_K_HEAVY, WPR_K_FOLD, WPR_K_ADD, WPR_K_COUNT_ };
enum { WPR_S_ERR = WAP_S_ERR, WPR_S_NHEAVY = WAP_S_NCHUNK, WPR_S_N = WAP_S_N };

struct WprLds {
    union {
        WapLds ap;                          // valid, bounds
        double part[WPR_BLOCK];             // heavy: the lanes' shares
        unsigned int flag[WPR_BLOCK];       // bins: 1: a wave-regime bin
    };
    long long item[WPR_WAVES];              // heavy: the wave's bin, -1: none
    unsigned int cnt[WPR_WAVES];
};

struct WprArgs {
    WapArgs ap;                             // the two run lists, region[], scalars, default_value
    long long width;
    long long r0, nr;                       // the batch: regions [r0, r0 + nr)
    double *rows;                           // [nr * width] the batch's rows
    unsigned long long *hmask;              // [4 per workgroup of the bins pass] its wave-regime bins
    long long *hcnt;                        // [workgroups] their number, then the number before the workgroup
    long long hblocks, n_heavy;
    long long fold_n, fold_s;               // fold: rows of the batch, the distance of the rows merged first
    double *add_dst;                        // add: dst = a + b, or b when a is null
    const double *add_a, *add_b;
};

// ---- the reference's rounding ----
WCV_DEV long long wpr_r(double c, long long i) { return (long long) round((double) i * c); }

// the smallest i in [0, L] with r(i) >= j, L + 1 when there is none
WCV_DEV long long wpr_b(double c, long long L, long long j) {
    if (j <= 0) return 0;
    const double e = ceil(((double) j - 0.5) / c);
    long long i = e < 0 ? 0 : e > (double) (L + 1) ? L + 1 : (long long) e;
    while (i > 0 && wpr_r(c, i - 1) >= j) i--;
    while (i <= L && wpr_r(c, i) < j) i++;
    return i;
}

struct WprBin {
    long long rs, rf, lo, hi;               // the region and its runs
    long long bj, bj1;                      // b_j, b_{j+1} (relative)
    long long x0, x1;                       // the positions whose value the bin takes (absolute); the last is apart
    long long k0, k1;                       // runs [k0, k1) meet [x0, x1); events k0 .. k1
    double c, nlast;
    long long W;
};

WCV_DEV WprBin wpr_bin(const WprArgs &a, long long i, long long j) {
    WprBin b;
    const WapRegion rg = a.ap.region[i];
    b.rs = a.ap.r_start[i]; b.rf = a.ap.r_finish[i];
    b.lo = rg.lo; b.hi = rg.lo + rg.nruns;
    b.W = a.width;
    const long long L = b.rf - b.rs;
    b.c = (double) b.W / (double) L;
    b.bj = wpr_b(b.c, L, j);
    b.bj1 = wpr_b(b.c, L, j + 1);
    const long long p1 = b.bj1 < L ? b.bj1 : L;
    long long p0 = b.bj < b.bj1 ? b.bj : b.bj - 1;
    if (p0 > L) p0 = L;
    b.x0 = b.rs + p0; b.x1 = b.rs + p1;
    b.nlast = 1.0;
    if (p1 > p0) {
        const long long ra = wpr_r(b.c, p1 - 1), rb = wpr_r(b.c, p1);
        long long fin = rb > ra + 1 ? rb : ra + 1;
        if (fin > b.W) fin = b.W;
        b.nlast = (double) (fin - ra);
    }
    long long q0 = b.lo, q1 = b.hi;         // the first run with finish > x0
    while (q0 < q1) { const long long mid = (q0 + q1) >> 1; if ((long long) a.ap.finish[mid] > b.x0) q1 = mid; else q0 = mid + 1; }
    b.k0 = q0;
    q1 = b.hi;                              // the first run from there on with start >= x1
    while (q0 < q1) { const long long mid = (q0 + q1) >> 1; if ((long long) a.ap.start[mid] >= b.x1) q1 = mid; else q0 = mid + 1; }
    b.k1 = q0;
    return b;
}

// event k of a bin: the uncovered stretch before run k (after the last run: up to rf), then, for k < k1, the piece of run k
WCV_DEV void wpr_event(const WprArgs &a, const WprBin &b, long long k, double &acc) {
    const double d = a.ap.default_value;
    if (d == d) {
        long long pe = b.rs, ge = b.rf;
        if (k > b.lo) { pe = a.ap.finish[k - 1]; if (pe > b.rf) pe = b.rf; }
        if (k < b.hi) { ge = a.ap.start[k]; if (ge < b.rs) ge = b.rs; }
        const long long ga = pe - b.rs, gb = ge - b.rs;
        if (gb > ga && ga < b.bj1 && (gb >= b.bj1 || ga >= b.bj)) {
            const long long ra = wpr_r(b.c, ga), rb = wpr_r(b.c, gb);
            long long fin = rb > ra + 1 ? rb : ra + 1;
            if (fin > b.W) fin = b.W;
            acc += d / (double) (fin - ra);
        }
    }
    if (k >= b.k1) return;
    const double v = wap_value(a.ap, k);
    if (!(v == v)) return;
    long long u = a.ap.start[k], w = a.ap.finish[k];
    if (u < b.x0) u = b.x0;
    if (w > b.x1) w = b.x1;
    if (w <= u) return;
    if (w == b.x1) {                        // (the last position of the bin's range: its own divisor)
        if (w - u > 1) acc += (double) (w - u - 1) * v;
        acc += v / b.nlast;
    } else {
        acc += (double) (w - u) * v;
    }
}

// share t of n: a contiguous run of the bin's events, in order
WCV_DEV double wpr_share(const WprArgs &a, const WprBin &b, int t, int n) {
    const long long nev = b.k1 - b.k0 + 1, per = (nev + n - 1) / n;
    long long e0 = b.k0 + (long long) t * per, e1 = e0 + per;
    if (e1 > b.k1 + 1) e1 = b.k1 + 1;
    double acc = 0.0;
    for (long long k = e0; k < e1; k++) wpr_event(a, b, k, acc);
    return acc;
}

WCV_DEV bool wpr_is_heavy(const WprBin &b) { return b.k1 - b.k0 > WPR_SMALL; }

// ---- bounds ----
WCV_DEV void wpr_bounds_block(const WprArgs &a, long long tile, WprLds *lds) {
    const WrgArgs r = wap_as_region(a.ap);
    wrg_window(r, tile, &lds->ap.rg);
    WCV_LANES(l) {
        const WrgMask m = wrg_tile_mask(r, &lds->ap.rg);
        for (int q = 0; q < WAP_PER_LANE; q++) {
            const long long i = tile * WAP_TILE + (long long) l * WAP_PER_LANE + q;
            if (i >= a.ap.n_r) break;
            long long lo, hi;
            wrg_span(r, m, i, wcv_seg_of(a.ap.r_seg_off, a.ap.n_seg, i), &lo, &hi);
            if (hi < lo) hi = lo;
            WapRegion rg;
            rg.lo = lo; rg.nruns = (int) (hi - lo); rg.cbase = 0;
            a.ap.region[i] = rg;
        }
    }
}

// ---- bins: lane l of workgroup b has item 256 b + l = (region r0 + item / W, bin item % W) ----
WCV_DEV void wpr_bins_block(const WprArgs &a, long long block, WprLds *lds) {
    WCV_LANES(l) {
        const long long item = block * WPR_BLOCK + l;
        unsigned int heavy = 0;
        if (item < a.nr * a.width) {
            const unsigned int q = (unsigned int) item / (unsigned int) a.width;         // (a batch has fewer than 2^31 bins)
            const WprBin b = wpr_bin(a, a.r0 + q, item - (long long) q * a.width);
            if (wpr_is_heavy(b)) heavy = 1;
            else a.rows[item] = wpr_share(a, b, 0, 1);
        }
        lds->flag[l] = heavy;
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (l < WPR_WAVES) {
            unsigned long long m = 0;
            for (int k = 0; k < WPR_WAVE; k++) if (lds->flag[l * WPR_WAVE + k]) m |= 1ull << k;
            a.hmask[block * WPR_WAVES + l] = m;
            lds->cnt[l] = (unsigned int) wcv_popc(m);
        }
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (l == 0) {
            long long n = 0;
            for (int k = 0; k < WPR_WAVES; k++) n += lds->cnt[k];
            a.hcnt[block] = n;
        }
    }
}

// wave-regime bin q of the batch (hcnt scanned) -> its item
WCV_DEV long long wpr_locate(const WprArgs &a, long long q) {
    long long b0 = 0, b1 = a.hblocks;           // hcnt[b0] <= q < hcnt[b1]
    while (b1 - b0 > 1) { const long long mid = (b0 + b1) >> 1; if (a.hcnt[mid] <= q) b0 = mid; else b1 = mid; }
    long long left = q - a.hcnt[b0];
    for (int w = 0; w < WPR_WAVES; w++) {
        unsigned long long m = a.hmask[b0 * WPR_WAVES + w];
        const int c = wcv_popc(m);
        if (left >= c) { left -= c; continue; }
        for (int k = 0; k < WPR_WAVE; k++)
            if ((m >> k) & 1ull) { if (left == 0) return b0 * WPR_BLOCK + w * WPR_WAVE + k; left--; }
    }
    return -1;
}

// ---- heavy: wave w of workgroup b sums wave-regime bin 4 b + w ----
WCV_DEV void wpr_heavy_block(const WprArgs &a, long long block, WprLds *lds) {
    WCV_LANES(l) {
        const int w = l / WPR_WAVE, t = l % WPR_WAVE;
        const long long q = block * WPR_WAVES + w;
        double acc = 0.0;
        long long item = -1;
        if (q < a.n_heavy) item = wpr_locate(a, q);
        if (item >= 0) {
            const unsigned int i = (unsigned int) item / (unsigned int) a.width;
            acc = wpr_share(a, wpr_bin(a, a.r0 + i, item - (long long) i * a.width), t, WPR_WAVE);
        }
        lds->part[l] = acc;
        if (t == 0) lds->item[w] = item;
    }
    for (int s = 1; s < WPR_WAVE; s <<= 1) {
        WCV_SYNC();
        WCV_LANES(l) {
            if ((l & (2 * s - 1)) == 0) lds->part[l] += lds->part[l + s];
        }
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (l % WPR_WAVE == 0 && lds->item[l / WPR_WAVE] >= 0) a.rows[lds->item[l / WPR_WAVE]] = lds->part[l];
    }
}

// ---- fold: rows g 8 s + t s (t = 0 .. 7) of the batch into the first of them; a row without a partner is carried ----
WCV_DEV void wpr_fold_block(const WprArgs &a, long long block, WprLds *) {
    WCV_LANES(l) {
        const long long item = block * WPR_BLOCK + l, groups = (a.fold_n + WPR_FOLD * a.fold_s - 1) / (WPR_FOLD * a.fold_s);
        if (item >= groups * a.width) continue;
        const long long g = (unsigned int) item / (unsigned int) a.width, j = item - g * a.width, first = g * WPR_FOLD * a.fold_s;
        double x[WPR_FOLD];
        bool e[WPR_FOLD];
#pragma unroll
        for (int t = 0; t < WPR_FOLD; t++) {
            const long long row = first + t * a.fold_s;
            e[t] = row < a.fold_n;
            x[t] = e[t] ? a.rows[row * a.width + j] : 0.0;
        }
#pragma unroll
        for (int st = 1; st < WPR_FOLD; st <<= 1) {
#pragma unroll
            for (int t = 0; t < WPR_FOLD; t += 2 * st)
                if (e[t + st]) x[t] += x[t + st];
        }
        a.rows[first * a.width + j] = x[0];
    }
}

WCV_DEV void wpr_add_block(const WprArgs &a, long long block, WprLds *) {
    WCV_LANES(l) {
        const long long j = block * WPR_BLOCK + l;
        if (j < a.width) a.add_dst[j] = a.add_a ? a.add_a[j] + a.add_b[j] : a.add_b[j];
    }
}

WCV_DEV void wpr_run_block(int kernel, const WprArgs &a, long long block, WprLds *lds) {
    switch (kernel) {
    case WPR_K_VALID_D: wap_valid_block(a.ap, false, block, &lds->ap); break;
    case WPR_K_VALID_R: wap_valid_block(a.ap, true, block, &lds->ap); break;
    case WPR_K_BOUNDS: wpr_bounds_block(a, block, lds); break;
    case WPR_K_BINS: wpr_bins_block(a, block, lds); break;
    case WPR_K_HEAVY: wpr_heavy_block(a, block, lds); break;
    case WPR_K_FOLD: wpr_fold_block(a, block, lds); break;
    case WPR_K_ADD: wpr_add_block(a, block, lds); break;
    default: break;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The door, written once over a Launcher: the one of wt_cover.h (alloc, release, zero, to_host, to_device, run over WcvArgs)
// with    bool run_profile(int kernel, long long blocks, const WprArgs &a)     and     bool sync()
// batch: regions per batch, 0: the default (rounded down to a power of two, at least 1).
// Return value: 0 fine, 1 bad argument, 2 launcher failure (the WTAMD_* codes).  Nothing is written to profile unless the
// value is 0.
// ---------------------------------------------------------------------------------------------------------------------
#ifndef WCV_NO_HOST

template <class L>
static int wpr_profile(L &l, long long n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish, const void *value,
                       int value_is_f64, const int64_t *r_seg_off, const int32_t *r_start, const int32_t *r_finish, long long width,
                       double default_value, unsigned int flags, long long batch, double *profile, const char **why) {
    const bool sum = (flags & WPR_SUM) != 0;
    WprArgs a = {};
    a.width = width;
    a.ap.n_seg = n_seg;
    a.ap.start = start; a.ap.finish = finish; a.ap.value = value; a.ap.value_is_f64 = value_is_f64;
    a.ap.r_start = r_start; a.ap.r_finish = r_finish;
    a.ap.default_value = default_value;
    if (const int rc = wap_open_check(a.ap, seg_off, r_seg_off, (flags & ~WPR_SUM) || width < 1 || width >= (1ll << 31) || batch < 0, profile, sum, why))
        return rc;
    const long long n_r = a.ap.n_r;
    if (n_r >= (1ll << 31)) { *why = "more than 2^31 - 1 regions"; return 1; }
    WcvScope<L> sc(l);
    if (const int rc = wap_open(l, sc, a.ap, seg_off, r_seg_off,
                                [&](bool regions, long long blocks) { return l.run_profile(regions ? WPR_K_VALID_R : WPR_K_VALID_D, blocks, a); }, why))
        return rc;
    long long h_sc[WPR_S_N];
    if (n_r == 0) {
        if (sum && (!l.zero(profile, sizeof(double) * (size_t) width) || !l.sync())) { *why = "copy"; return 2; }
        return 0;
    }
    // the batch: a power of two of regions
    long long want = batch > 0 ? batch : WPR_BATCH_DOUBLES / width, B = 1;
    while (2 * B <= want && B < n_r && 2 * B * width < (1ll << 31)) B *= 2;       // (fewer than 2^31 bins: the passes divide in 32 bits)
    const long long batches = (n_r + B - 1) / B, items = B * width, blocks = wcv_blocks(items, WPR_BLOCK);
    int levels = 2;
    for (long long q = batches; q > 1; q >>= 1) levels++;
    a.hblocks = blocks;
    double *rows = nullptr, *stack = nullptr;
    if (!sc.get(&a.ap.region, (size_t) n_r) || !sc.get(&a.hmask, (size_t) blocks * WPR_WAVES) || !sc.get(&a.hcnt, (size_t) blocks) ||
        (sum && (!sc.get(&rows, (size_t) items) || !sc.get(&stack, (size_t) levels * (size_t) width))))
        { *why = "device memory"; return 2; }
    if (!l.run_profile(WPR_K_BOUNDS, wcv_blocks(n_r, WAP_TILE), a)) { *why = "bounds pass"; return 2; }
    std::vector<char> full((size_t) levels, 0);          // the binary counter: stack row q holds a node of level q above the batch
    const long long wblocks = wcv_blocks(width, WPR_BLOCK);
    for (long long r0 = 0; r0 < n_r; r0 += B) {
        a.r0 = r0; a.nr = n_r - r0 < B ? n_r - r0 : B;
        a.rows = sum ? rows : profile + r0 * width;
        a.hblocks = wcv_blocks(a.nr * width, WPR_BLOCK);
        WcvArgs s = {};
        s.scan = a.hcnt; s.scan_n = a.hblocks; s.scan_init = nullptr; s.scan_total = &a.ap.scalars[WPR_S_NHEAVY];
        if (!l.run_profile(WPR_K_BINS, a.hblocks, a) || !l.run(WCV_K_SCAN_SUM, 1, s) || !l.to_host(h_sc, a.ap.scalars, sizeof h_sc))
            { *why = "bins pass"; return 2; }
        a.n_heavy = h_sc[WPR_S_NHEAVY];
        if (!l.run_profile(WPR_K_HEAVY, wcv_blocks(a.n_heavy, WPR_WAVES), a)) { *why = "heavy pass"; return 2; }
        if (!sum) continue;
        a.fold_n = a.nr;
        for (a.fold_s = 1; a.fold_s < a.nr; a.fold_s *= WPR_FOLD)
            if (!l.run_profile(WPR_K_FOLD, wcv_blocks(wcv_blocks(a.nr, WPR_FOLD * a.fold_s) * width, WPR_BLOCK), a)) { *why = "fold pass"; return 2; }
        int q = 0;                                          // rows[0 .. W) is the batch's node: carry it up the counter
        for (; full[(size_t) q]; q++) {
            a.add_dst = rows; a.add_a = stack + (size_t) q * (size_t) width; a.add_b = rows;
            if (!l.run_profile(WPR_K_ADD, wblocks, a)) { *why = "add pass"; return 2; }
            full[(size_t) q] = 0;
        }
        a.add_dst = stack + (size_t) q * (size_t) width; a.add_a = nullptr; a.add_b = rows;
        if (!l.run_profile(WPR_K_ADD, wblocks, a)) { *why = "add pass"; return 2; }
        full[(size_t) q] = 1;
    }
    if (sum) {                                              // what is left in the counter, the later (smaller) nodes first
        const double *carry = nullptr;
        for (int q = 0; q < levels; q++) {
            if (!full[(size_t) q]) continue;
            double *row = stack + (size_t) q * (size_t) width;
            if (carry) {
                a.add_dst = row; a.add_a = row; a.add_b = carry;
                if (!l.run_profile(WPR_K_ADD, wblocks, a)) { *why = "add pass"; return 2; }
            }
            carry = row;
        }
        a.add_dst = profile; a.add_a = nullptr; a.add_b = carry;
        if (!l.run_profile(WPR_K_ADD, wblocks, a)) { *why = "add pass"; return 2; }
    }
    if (!l.sync()) { *why = "synchronisation"; return 2; }
    return 0;
}

#endif  // WCV_NO_HOST

// The same rules on the host, without a device (a translation unit compiled with -DWT_EMU: the arithmetic above is then plain
// C++): one segment pair, one forward sweep for the regions' run ranges (lo only moves forward), every bin by the functions
// above -- the wave regime's 64 shares one after the other, merged in the same order --, the sum by the same tree.
#ifdef WT_EMU
#include <vector>

static double wpr_bin_host(const WprArgs &a, const WprBin &b) {
    if (!wpr_is_heavy(b)) return wpr_share(a, b, 0, 1);
    double part[WPR_WAVE];
    for (int t = 0; t < WPR_WAVE; t++) part[t] = wpr_share(a, b, t, WPR_WAVE);
    for (int s = 1; s < WPR_WAVE; s <<= 1)
        for (int t = 0; t < WPR_WAVE; t += 2 * s) part[t] += part[t + s];
    return part[0];
}

static int wpr_profile_host(long long n, const int32_t *start, const int32_t *finish, const double *value, long long n_r,
                            const int32_t *r_start, const int32_t *r_finish, long long width, double default_value, unsigned int flags,
                            double *profile) {
    const bool sum = (flags & WPR_SUM) != 0;
    if (n < 0 || n_r < 0 || (flags & ~WPR_SUM) || width < 1 || width >= (1ll << 31) || (n > 0 && (!start || !finish || !value)) ||
        (n_r > 0 && (!r_start || !r_finish)) || ((n_r > 0 || sum) && !profile))
        return 1;
    for (long long i = 0; i < n; i++) if (start[i] < 0 || start[i] >= finish[i] || (i > 0 && finish[i - 1] > start[i])) return 1;
    for (long long i = 0; i < n_r; i++) if (r_start[i] < 0 || r_start[i] >= r_finish[i] || (i > 0 && r_start[i - 1] > r_start[i])) return 1;
    WprArgs a = {};
    WapRegion rg = {};
    a.width = width;
    a.ap.start = start; a.ap.finish = finish; a.ap.value = value; a.ap.value_is_f64 = 1; a.ap.default_value = default_value;
    a.ap.region = &rg;
    std::vector<std::vector<double>> node;      // the binary counter of the sum: node[q] a row of level q, empty: none
    std::vector<double> row((size_t) width);
    long long lo = 0;
    for (long long i = 0; i < n_r; i++) {
        const int32_t rs = r_start[i], rf = r_finish[i];
        while (lo < n && finish[lo] <= rs) lo++;
        long long hi = lo;
        while (hi < n && start[hi] < rf) hi++;
        rg.lo = lo; rg.nruns = (int) (hi - lo);
        a.ap.r_start = r_start + i; a.ap.r_finish = r_finish + i;
        double *out = sum ? row.data() : profile + i * width;
        for (long long j = 0; j < width; j++) out[j] = wpr_bin_host(a, wpr_bin(a, 0, j));
        if (!sum) continue;
        std::vector<double> carry = row;
        size_t q = 0;
        for (; q < node.size() && !node[q].empty(); q++) {
            for (long long j = 0; j < width; j++) carry[(size_t) j] = node[q][(size_t) j] + carry[(size_t) j];
            node[q].clear();
        }
        if (q == node.size()) node.emplace_back();
        node[q] = carry;
    }
    if (sum) {
        std::vector<double> carry;
        for (size_t q = 0; q < node.size(); q++) {
            if (node[q].empty()) continue;
            if (!carry.empty()) for (long long j = 0; j < width; j++) node[q][(size_t) j] += carry[(size_t) j];
            carry = node[q];
        }
        for (long long j = 0; j < width; j++) profile[j] = carry.empty() ? 0.0 : carry[(size_t) j];
    }
    return 0;
}
#endif  // WT_EMU

#endif  // WT_PROFILE_H_
