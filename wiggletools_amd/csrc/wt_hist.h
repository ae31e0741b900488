// wt_hist.h -- value histograms of whole run lists (device + -DWT_EMU): the reference's histogram() (src/plots.c:77-223; the
// parser's `histogram (output) (width) (iterator_list)`).  This header is the single source of the logic.  It is compiled
//   * by hipcc for gfx950 inside csrc/wt_hist.hip (the product),
//   * by g++ with -DWT_EMU inside tests/hist_emu.cpp, which runs the workgroups of every pass one after the other in any order
//     on the CPU, and
//   * as plain C++ inside the drop-in layer (csrc/wt_abi_hist.h), which uses the host sweep at the end.
//
// Input (the layout of wtamd_runs_map): n_seg segments, seg_off[n_seg + 1], start / finish / value, and seg_row[n_seg], the
// histogram row (0 .. n_rows - 1) of every segment.  The runs need be neither sorted nor disjoint: the reference histograms
// raw iterators and counts overlapping intervals once each.  The only rule per run is start < finish; no value is infinite.
//
// THE RULE.  lo, hi: the minimum and maximum of all non-NaN values of all rows.  A run with a NaN value is skipped.  A run of
// value v and length L = finish - start adds L to column c of its row: c = 0 when lo == hi, otherwise
//     c = (int) ((v - lo) * (double) width / (hi - lo))          subtract, multiply, ONE IEEE division, in double, in that order
// and c == width becomes width - 1 (the reference's insertIntoHistogram, plots.c:148-153).  f32 values are widened first.  A
// quotient that is not below width (v == hi; or a span hi - lo or a product that overflows double) lands in width - 1.
//
// EXACT IN ANY ORDER.  The two-pass form needs none of the reference's re-binning.  The counters are unsigned 64-bit integers
// in LDS and in global memory (a segment has fewer than 2^31 runs shorter than 2^31: one column can pass 2^32), so the sums
// are those of integers and do not depend on the order in which workgroups, waves and atomics happen to run; the last pass
// converts them to double, exact below 2^53.  The minimum and maximum of a set do not depend on an order either, once a zero
// extreme is delivered as +0.0 (x + 0.0).
//
//   range   WHS_SHARE runs per workgroup: start < finish, no infinite value (counted in WHS_S_ERR), and the minimum / maximum of
//           the non-NaN values as order-preserving 64-bit keys: a tree in LDS, then one atomicMin and one atomicMax per workgroup
//   load    (WTAMD_HIST_ACCUMULATE) the caller's matrix back into the counters; a cell that is not a whole number in [0, 2^53)
//           is counted in WHS_S_ERR
//   bins    workgroups are dealt to rows by a host table (whs_table): a workgroup takes at most WHS_SHARE consecutive runs of
//           ONE row and accumulates into `width` counters in LDS, which it then flushes, the non-zero ones, with one global
//           64-bit atomic each.  Real tracks are skewed (most of a coverage track is one value), so a wave does not send 64
//           same-address atomics: whs_wave_add combines inside the wave first.  All active lanes in one column: one sum, one
//           atomic (the wave-uniform path).  Otherwise the columns of the first WHS_PEEL leaders are looked at: one held by
//           WHS_COMBINE_MIN lanes or more is summed and added by its leader (the sum costs 12 cross-lane moves: a column of a
//           few lanes is cheaper as it is), and what is then left goes out as plain atomics, one per lane.
//   binsg   width > WHS_LDS_WIDTH: the same template accumulating directly in the global counters
//   finish  u64 -> double into the caller's matrix
#ifndef WT_HIST_H_
#define WT_HIST_H_

#include <math.h>
#include <string.h>

#include <vector>

#include "wt_cover.h"

#define WHS_BLOCK WCV_BLOCK
#define WHS_RUNS_PER_LANE 64                    // runs one lane of the range / bins passes takes
#define WHS_SHARE (WHS_BLOCK * WHS_RUNS_PER_LANE)       // a workgroup's share of runs
#define WHS_BATCH 8                             // runs a lane loads before it uses the first (the loads are then in flight together)
#define WHS_LDS_WIDTH 4096                      // widest histogram row a workgroup keeps in LDS (32 KiB of counters)
#define WHS_WAVE 64
#define WHS_WAVES (WHS_BLOCK / WHS_WAVE)
#define WHS_PEEL 2                              // leaders' columns a wave looks at before it falls back to one atomic per lane
#define WHS_COMBINE_MIN 8                       // lanes in one column from which their sum is formed (below: one atomic each)
static_assert(WHS_RUNS_PER_LANE % WHS_BATCH == 0, "a lane's runs are whole batches");
#define WHS_MAX_CELLS (1ll << 40)               // n_rows x width of one call

#define WHS_RANGE_GIVEN 1u                      // WTAMD_HIST_RANGE_GIVEN
#define WHS_ACCUMULATE 2u                       // WTAMD_HIST_ACCUMULATE

enum { WHS_K_RANGE = 0, WHS_K_LOAD, WHS_K_BINS, WHS_K_BINSG, WHS_K_FINISH, WHS_K_COUNT_ };
enum { WHS_S_ERR = 0, WHS_S_MIN = 1, WHS_S_MAX = 2, WHS_S_N = 4 };

typedef unsigned long long whs_u64;

#ifdef WT_EMU
WCV_DEV void whs_addu64(whs_u64 *p, whs_u64 v) { *p += v; }
WCV_DEV void whs_minu64(whs_u64 *p, whs_u64 v) { if (v < *p) *p = v; }
WCV_DEV void whs_maxu64(whs_u64 *p, whs_u64 v) { if (v > *p) *p = v; }
#else
// (A minimum only falls and a maximum only rises: a plain look first spares the atomic that could not change anything -- all but
// the first few of a pass, which would otherwise queue on one address -- and a stale look only costs an atomic it did not need.)
WCV_DEV void whs_addu64(whs_u64 *p, whs_u64 v) { atomicAdd(p, v); }
WCV_DEV void whs_minu64(whs_u64 *p, whs_u64 v) { if (v < *(volatile whs_u64 *) p) atomicMin(p, v); }
WCV_DEV void whs_maxu64(whs_u64 *p, whs_u64 v) { if (v > *(volatile whs_u64 *) p) atomicMax(p, v); }
#endif

// A workgroup's LDS is an array of 64-bit words: WHS_LDS_WIDTH counters for the bins pass, 2 WHS_BLOCK keys (the lanes' minima,
// then their maxima) for the range pass, none for the others.  (The emulator's launcher wants a type.)
#define WHS_RANGE_WORDS (2 * WHS_BLOCK)
struct WhsLds {
    whs_u64 w[WHS_LDS_WIDTH];
};

// one workgroup of the bins pass (host-made)
struct WhsItem {
    long long r0;                               // its first run
    int count;                                  // its runs, 1 .. WHS_SHARE
    int row;
};

struct WhsArgs {
    const int32_t *start, *finish;
    const void *value;
    int value_is_f64;
    long long n;                                // runs
    int width, n_rows;
    long long cells;                            // n_rows x width
    double lo, hi;
    whs_u64 *scalars;                           // [WHS_S_N]
    whs_u64 *cnt;                               // [cells]
    double *hist;                               // [cells] the caller's
    const WhsItem *tab;
};

WCV_DEV double whs_value(const WhsArgs &a, long long i) {
    return a.value_is_f64 ? ((const double *) a.value)[i] : (double) ((const float *) a.value)[i];
}

// doubles to keys whose unsigned order is the doubles' order, and (on the host) back
WCV_DEV whs_u64 whs_key(double x) {
    whs_u64 b;
    memcpy(&b, &x, 8);
    return (b >> 63) ? ~b : b | (1ull << 63);
}
static inline double whs_unkey(whs_u64 k) {
    const whs_u64 b = (k >> 63) ? k & ~(1ull << 63) : ~k;
    double x;
    memcpy(&x, &b, 8);
    return x;
}

// the column of a non-NaN value inside [lo, hi]
WCV_DEV int whs_column(double v, double lo, double hi, int width) {
    if (lo == hi) return 0;
    const double q = (v - lo) * (double) width / (hi - lo);
    return q < (double) width ? (int) q : width - 1;
}

// ---- range: validation and the two extremes ----
WCV_DEV void whs_range_block(const WhsArgs &a, long long block, whs_u64 *key) {
    WCV_LANES(l) {
        whs_u64 mn = ~0ull, mx = 0ull;
        long long bad = 0;
        for (int k0 = 0; k0 < WHS_RUNS_PER_LANE; k0 += WHS_BATCH) {
            int32_t s[WHS_BATCH], f[WHS_BATCH];
            double v[WHS_BATCH];
#pragma unroll
            for (int k = 0; k < WHS_BATCH; k++) {           // (past the end: the last run again, not looked at)
                const long long i = block * WHS_SHARE + (long long) (k0 + k) * WHS_BLOCK + l, ii = i < a.n ? i : a.n - 1;
                s[k] = a.start[ii]; f[k] = a.finish[ii]; v[k] = whs_value(a, ii);
            }
#pragma unroll
            for (int k = 0; k < WHS_BATCH; k++) {
                if (block * WHS_SHARE + (long long) (k0 + k) * WHS_BLOCK + l >= a.n) continue;
                if (s[k] >= f[k]) bad++;
                if (v[k] != v[k]) continue;
                if (v[k] - v[k] != 0.0) { bad++; continue; }          // infinite
                const whs_u64 x = whs_key(v[k] + 0.0);
                if (x < mn) mn = x;
                if (x > mx) mx = x;
            }
        }
        if (bad) whs_addu64(&a.scalars[WHS_S_ERR], (whs_u64) bad);
        key[l] = mn;
        key[WHS_BLOCK + l] = mx;
    }
    for (int s = WHS_BLOCK / 2; s > 0; s >>= 1) {
        WCV_SYNC();
        WCV_LANES(l) {
            if (l < s) {
                if (key[l + s] < key[l]) key[l] = key[l + s];
                if (key[WHS_BLOCK + l + s] > key[WHS_BLOCK + l]) key[WHS_BLOCK + l] = key[WHS_BLOCK + l + s];
            }
        }
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (l == 0 && key[0] <= key[WHS_BLOCK]) {           // (a workgroup of NaN runs has nothing to say)
            whs_minu64(&a.scalars[WHS_S_MIN], key[0]);
            whs_maxu64(&a.scalars[WHS_S_MAX], key[WHS_BLOCK]);
        }
    }
}

// ---- load: the caller's matrix into the counters ----
WCV_DEV void whs_load_block(const WhsArgs &a, long long block) {
    WCV_LANES(l) {
        const long long i = block * WHS_BLOCK + l;
        if (i >= a.cells) continue;
        const double x = a.hist[i];
        if (!(x >= 0.0 && x < 9007199254740992.0) || x != floor(x)) { whs_addu64(&a.scalars[WHS_S_ERR], 1); continue; }
        a.cnt[i] = (whs_u64) x;
    }
}

// ---- finish: the counters into the caller's matrix ----
WCV_DEV void whs_finish_block(const WhsArgs &a, long long block) {
    WCV_LANES(l) {
        const long long i = block * WHS_BLOCK + l;
        if (i < a.cells) a.hist[i] = (double) a.cnt[i];
    }
}

// One step of a wave: lane t adds len to cnt[col] (col < 0: it has nothing).  Lanes that hold the same column add their
// lengths and one of them issues the add.  The device form and, beside it, the emulator's over the 64 lanes' values.
#ifndef WT_EMU
WCV_DEV whs_u64 whs_wave_sum(whs_u64 x) {
    for (int s = WHS_WAVE / 2; s > 0; s >>= 1) x += __shfl_xor(x, s, WHS_WAVE);
    return x;
}
WCV_DEV void whs_wave_add(whs_u64 *cnt, int col, unsigned int len) {
    const int t = (int) (threadIdx.x % WHS_WAVE);
    whs_u64 todo = __ballot(col >= 0);
    for (int peel = 0; peel < WHS_PEEL && todo != 0; peel++) {
        const int leader = __ffsll((unsigned long long) todo) - 1;
        const int c = __shfl(col, leader, WHS_WAVE);
        const bool mine = ((todo >> t) & 1ull) && col == c;
        const whs_u64 m = __ballot(mine);
        if (__popcll(m) >= WHS_COMBINE_MIN) {               // a column worth a sum: its leader adds it (all lanes: the wave-uniform path)
            const whs_u64 sum = whs_wave_sum(mine ? (whs_u64) len : 0ull);
            if (t == leader) whs_addu64(&cnt[c], sum);
        } else if (mine) whs_addu64(&cnt[col], (whs_u64) len);
        todo &= ~m;
    }
    if ((todo >> t) & 1ull) whs_addu64(&cnt[col], (whs_u64) len);     // spread: what is left goes out lane by lane
}
#else
static inline void whs_wave_add_emu(whs_u64 *cnt, const int *col, const unsigned int *len) {
    whs_u64 todo = 0;
    for (int t = 0; t < WHS_WAVE; t++) if (col[t] >= 0) todo |= 1ull << t;
    for (int peel = 0; peel < WHS_PEEL && todo != 0; peel++) {
        const int leader = __builtin_ffsll((long long) todo) - 1;
        const int c = col[leader];
        whs_u64 sum = 0, m = 0;
        for (int t = 0; t < WHS_WAVE; t++) if (((todo >> t) & 1ull) && col[t] == c) { m |= 1ull << t; sum += len[t]; }
        if (__builtin_popcountll(m) >= WHS_COMBINE_MIN) whs_addu64(&cnt[c], sum);
        else for (int t = 0; t < WHS_WAVE; t++) if ((m >> t) & 1ull) whs_addu64(&cnt[col[t]], (whs_u64) len[t]);
        todo &= ~m;
    }
    for (int t = 0; t < WHS_WAVE; t++) if ((todo >> t) & 1ull) whs_addu64(&cnt[col[t]], (whs_u64) len[t]);
}
#endif

// ---- bins: one workgroup, at most WHS_SHARE runs of one row ----
template <bool LDS>
WCV_DEV void whs_bins_block(const WhsArgs &a, long long block, whs_u64 *lds) {
    const WhsItem it = a.tab[block];
    whs_u64 *row = a.cnt + (long long) it.row * a.width;
    whs_u64 *cnt = LDS ? lds : row;
    if (LDS) {
        WCV_LANES(l) { for (int c = l; c < a.width; c += WHS_BLOCK) lds[c] = 0; }
        WCV_SYNC();
    }
    for (int k0 = 0; k0 < WHS_RUNS_PER_LANE; k0 += WHS_BATCH) {
        if (k0 * WHS_BLOCK >= it.count) break;              // (uniform over the workgroup)
#ifdef WT_EMU
        int ecol[WHS_BATCH][WHS_BLOCK];                     // (the emulator keeps the lanes' registers of the batch here)
        unsigned int elen[WHS_BATCH][WHS_BLOCK];
#endif
        WCV_LANES(l) {
            int32_t s[WHS_BATCH], f[WHS_BATCH];
            double v[WHS_BATCH];
#pragma unroll
            for (int k = 0; k < WHS_BATCH; k++) {           // (past the end: the last run again, not counted)
                const int j = (k0 + k) * WHS_BLOCK + l;
                const long long i = it.r0 + (j < it.count ? j : it.count - 1);
                s[k] = a.start[i]; f[k] = a.finish[i]; v[k] = whs_value(a, i);
            }
#pragma unroll
            for (int k = 0; k < WHS_BATCH; k++) {
                int col = -1;
                unsigned int len = 0;
                if ((k0 + k) * WHS_BLOCK + l < it.count && v[k] == v[k]) {
                    col = whs_column(v[k], a.lo, a.hi, a.width);
                    len = (unsigned int) ((long long) f[k] - (long long) s[k]);
                }
#ifndef WT_EMU
                whs_wave_add(cnt, col, len);
#else
                ecol[k][l] = col; elen[k][l] = len;
#endif
            }
        }
#ifdef WT_EMU
        for (int k = 0; k < WHS_BATCH; k++)
            for (int w = 0; w < WHS_WAVES; w++) whs_wave_add_emu(cnt, ecol[k] + w * WHS_WAVE, elen[k] + w * WHS_WAVE);
#endif
    }
    if (LDS) {
        WCV_SYNC();
        WCV_LANES(l) {
            for (int c = l; c < a.width; c += WHS_BLOCK) { const whs_u64 x = lds[c]; if (x) whs_addu64(&row[c], x); }
        }
    }
}

// pass `kernel`, one workgroup; lds: its words (WHS_LDS_WIDTH for bins, WHS_RANGE_WORDS for range)
WCV_DEV void whs_run_words(int kernel, const WhsArgs &a, long long block, whs_u64 *lds) {
    switch (kernel) {
    case WHS_K_RANGE: whs_range_block(a, block, lds); break;
    case WHS_K_LOAD: whs_load_block(a, block); break;
    case WHS_K_BINS: whs_bins_block<true>(a, block, lds); break;
    case WHS_K_BINSG: whs_bins_block<false>(a, block, lds); break;
    case WHS_K_FINISH: whs_finish_block(a, block); break;
    default: break;
    }
}
WCV_DEV void whs_run_block(int kernel, const WhsArgs &a, long long block, WhsLds *lds) { whs_run_words(kernel, a, block, lds->w); }

// what every entry checks before it touches anything; "" when fine
static inline const char *whs_check(long long n_seg, const int64_t *seg_off, const int32_t *seg_row, int n_rows, const int32_t *start,
                                    const int32_t *finish, const void *value, int width, unsigned int flags, const double *range2, const double *hist) {
    if (n_seg < 0 || !seg_off || !range2 || !hist || (n_seg > 0 && !seg_row)) return "bad argument";
    if (width < 1) return "the width must be 1 or more";
    if (n_rows < 1) return "there must be a row";
    if ((long long) n_rows * width > WHS_MAX_CELLS) return "too many cells";
    if (flags & ~(WHS_RANGE_GIVEN | WHS_ACCUMULATE)) return "unknown flag";
    if ((flags & WHS_ACCUMULATE) && !(flags & WHS_RANGE_GIVEN)) return "WTAMD_HIST_ACCUMULATE needs WTAMD_HIST_RANGE_GIVEN";
    if ((flags & WHS_RANGE_GIVEN) && (!(range2[0] <= range2[1]) || range2[0] - range2[0] != 0.0 || range2[1] - range2[1] != 0.0))
        return "the given range is NaN, infinite or inverted";
    if (n_seg > 0 && seg_off[0] != 0) return "bad argument";
    for (long long g = 0; g < n_seg; g++) {
        if (seg_off[g + 1] < seg_off[g]) return "segment offsets decrease";
        if (seg_row[g] < 0 || seg_row[g] >= n_rows) return "a segment's row is outside [0, n_rows)";
    }
    const long long n = n_seg ? (long long) seg_off[n_seg] : 0;
    if (n >= (1ll << 31) || (n > 0 && (!start || !finish || !value))) return "bad argument";
    return "";
}

// ---------------------------------------------------------------------------------------------------------------------
// The door, written once over a Launcher: the one of wt_cover.h (alloc, release, zero, to_host, to_device) with
//     bool run_hist(int kernel, long long blocks, const WhsArgs &a)     and     bool sync()
// Return value: 0 fine, 1 bad argument, 2 launcher failure.  Nothing is written to hist or range2 unless the value is 0.
// Temporary memory: 8 bytes per cell, 16 bytes per workgroup of the bins pass (one per WHS_SHARE runs of a stretch of
// segments of one row), 32 bytes of scalars.
// ---------------------------------------------------------------------------------------------------------------------
#ifndef WCV_NO_HOST

// the workgroups of the bins pass: consecutive segments of one row are one stretch, cut into shares
static inline void whs_table(long long n_seg, const int64_t *seg_off, const int32_t *seg_row, std::vector<WhsItem> *tab) {
    long long g = 0;
    while (g < n_seg) {
        long long e = g + 1;
        while (e < n_seg && seg_row[e] == seg_row[g]) e++;
        for (long long r = seg_off[g]; r < (long long) seg_off[e]; r += WHS_SHARE) {
            const long long left = (long long) seg_off[e] - r;
            tab->push_back(WhsItem{r, (int) (left < WHS_SHARE ? left : WHS_SHARE), (int) seg_row[g]});
        }
        g = e;
    }
}

template <class L>
static int whs_door(L &l, long long n_seg, const int64_t *seg_off, const int32_t *seg_row, int n_rows, const int32_t *start, const int32_t *finish,
                    const void *value, int value_is_f64, int width, unsigned int flags, double *range2, double *hist, const char **why) {
    *why = whs_check(n_seg, seg_off, seg_row, n_rows, start, finish, value, width, flags, range2, hist);
    if (**why) return 1;
    WhsArgs a = {};
    a.start = start; a.finish = finish; a.value = value; a.value_is_f64 = value_is_f64;
    a.n = n_seg ? (long long) seg_off[n_seg] : 0;
    a.width = width; a.n_rows = n_rows; a.cells = (long long) n_rows * width;
    a.hist = hist;
    WcvScope<L> sc(l);
    if (!sc.get(&a.scalars, (size_t) WHS_S_N) || !sc.get(&a.cnt, (size_t) a.cells)) { *why = "device memory"; return 2; }
    whs_u64 h_sc[WHS_S_N] = {0, ~0ull, 0, 0};
    if (!l.to_device(a.scalars, h_sc, sizeof h_sc) || !l.run_hist(WHS_K_RANGE, wcv_blocks(a.n, WHS_SHARE), a) || !l.to_host(h_sc, a.scalars, sizeof h_sc))
        { *why = "range pass"; return 2; }
    if (h_sc[WHS_S_ERR]) { *why = "a run with start >= finish, or an infinite value"; return 1; }
    const bool any = h_sc[WHS_S_MIN] <= h_sc[WHS_S_MAX];
    double lo = any ? whs_unkey(h_sc[WHS_S_MIN]) : (double) NAN, hi = any ? whs_unkey(h_sc[WHS_S_MAX]) : (double) NAN;
    if (flags & WHS_RANGE_GIVEN) {
        if (any && (lo < range2[0] || hi > range2[1])) { *why = "a value lies outside the given range"; return 1; }
        lo = range2[0] + 0.0; hi = range2[1] + 0.0;
    }
    a.lo = lo; a.hi = hi;
    const long long cblocks = wcv_blocks(a.cells, WHS_BLOCK);
    if (flags & WHS_ACCUMULATE) {
        if (!l.run_hist(WHS_K_LOAD, cblocks, a) || !l.to_host(h_sc, a.scalars, sizeof h_sc)) { *why = "load pass"; return 2; }
        if (h_sc[WHS_S_ERR]) { *why = "WTAMD_HIST_ACCUMULATE: hist does not hold whole numbers below 2^53"; return 1; }
    } else if (!l.zero(a.cnt, sizeof(whs_u64) * (size_t) a.cells)) { *why = "zero"; return 2; }
    if (any) {
        std::vector<WhsItem> tab;
        whs_table(n_seg, seg_off, seg_row, &tab);
        WhsItem *d_tab = nullptr;
        if (!sc.get(&d_tab, tab.size())) { *why = "device memory"; return 2; }
        a.tab = d_tab;
        if (!l.to_device(d_tab, tab.data(), sizeof(WhsItem) * tab.size()) ||
            !l.run_hist(width <= WHS_LDS_WIDTH ? WHS_K_BINS : WHS_K_BINSG, (long long) tab.size(), a)) { *why = "bins pass"; return 2; }
    }
    if (!l.run_hist(WHS_K_FINISH, cblocks, a) || !l.sync()) { *why = "finish pass"; return 2; }
    if (!(flags & WHS_RANGE_GIVEN)) { range2[0] = lo; range2[1] = hi; }
    return 0;
}

#endif  // WCV_NO_HOST

// The same rule on the host, without a device (a translation unit compiled with -DWT_EMU): one sweep for the range, one for
// the counters.  The same arguments, flags and refusals as the door's, hist in host memory; the same bits.
#ifdef WT_EMU

static int whs_host(long long n_seg, const int64_t *seg_off, const int32_t *seg_row, int n_rows, const int32_t *start, const int32_t *finish,
                    const double *value, int width, unsigned int flags, double *range2, double *hist) {
    if (*whs_check(n_seg, seg_off, seg_row, n_rows, start, finish, value, width, flags, range2, hist)) return 1;
    const long long n = n_seg ? (long long) seg_off[n_seg] : 0, cells = (long long) n_rows * width;
    whs_u64 mn = ~0ull, mx = 0ull;
    for (long long i = 0; i < n; i++) {
        const double v = value[i];
        if (start[i] >= finish[i] || (v == v && v - v != 0.0)) return 1;
        if (v != v) continue;
        const whs_u64 key = whs_key(v + 0.0);
        if (key < mn) mn = key;
        if (key > mx) mx = key;
    }
    const bool any = mn <= mx;
    double lo = any ? whs_unkey(mn) : (double) NAN, hi = any ? whs_unkey(mx) : (double) NAN;
    if (flags & WHS_RANGE_GIVEN) {
        if (any && (lo < range2[0] || hi > range2[1])) return 1;
        lo = range2[0] + 0.0; hi = range2[1] + 0.0;
    }
    std::vector<whs_u64> cnt((size_t) cells, 0ull);
    if (flags & WHS_ACCUMULATE)
        for (long long i = 0; i < cells; i++) {
            const double x = hist[i];
            if (!(x >= 0.0 && x < 9007199254740992.0) || x != floor(x)) return 1;
            cnt[(size_t) i] = (whs_u64) x;
        }
    for (long long g = 0; g < n_seg; g++)
        for (long long i = seg_off[g]; i < (long long) seg_off[g + 1]; i++) {
            const double v = value[i];
            if (v == v) cnt[(size_t) ((long long) seg_row[g] * width + whs_column(v, lo, hi, width))] += (whs_u64) ((long long) finish[i] - (long long) start[i]);
        }
    for (long long i = 0; i < cells; i++) hist[i] = (double) cnt[(size_t) i];
    if (!(flags & WHS_RANGE_GIVEN)) { range2[0] = lo; range2[1] = hi; }
    return 0;
}
#endif  // WT_EMU

#endif  // WT_HIST_H_
