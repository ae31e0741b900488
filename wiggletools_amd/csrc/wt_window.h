// wt_window.h -- the window operators over whole run lists (device + -DWT_EMU): the reference's BinningWiggleIterator
// (src/unaryOps.c:963-1036; the parser's `bin`) and SmoothWiggleIterator (:1039-1162; `smooth`).  This header is the single
// source of the logic.  It is compiled
//   * by hipcc for gfx950 inside csrc/wt_window.hip (the product),
//   * by g++ with -DWT_EMU inside tests/window_emu.cpp, which runs the workgroups of every pass one after the other in any
//     order on the CPU, and
//   * as plain C++ inside the drop-in layer (csrc/wt_abi_window.h), which uses the host sweeps at the end.
//
// Input (the layout of wtamd_runs_map): n_seg segments, seg_off[n_seg + 1], start / finish / value; inside a segment the runs
// are sorted, start < finish, DISJOINT (the reference puts its union in front of both operators) and start >= 1 (below 1 the
// reference's C division and its prefill do odd things: the drop-in serves such a chromosome by the reference's own protocol).
//
// BIN, width w.  The grid bins of a segment are [1 + k w, 1 + (k + 1) w); a bin is emitted, in order, iff a run intersects it
// (:990-996: continuing at the last finish and realigning land on the same grid); adjacent bins are not merged.  Its value
// starts at 0.0 and takes (double) covered * value of every intersecting run in order, then, when the default is not zero (NaN
// counts: C's truth) and the covered length is below w, (w - covered) * default.
//   OWNERSHIP.  Run i owns the bins it is the FIRST run to intersect: those above last_bin(i - 1).  Disjoint sorted runs have
//   non-decreasing last bins, so the owned bins of all runs in run order are the output in output order.
//   valid   one lane per run
//   count   the owned bins of 8 runs per lane, summed per workgroup; scan of the sums (wcv_scan_block of wt_cover.h)
//   cum     the exclusive scan per run, and the output offset of every segment
//   bins    ONE LANE PER OUTPUT BIN (a long run owning thousands of bins spreads over thousands of lanes): the workgroup finds
//           the runs its WWN_TILE bins belong to and, when they are at most WWN_WINDOW, stages their scanned counts in LDS;
//           a lane finds its owner by binary search there (in global memory otherwise), then walks forward from the owner
//           while run.start < bin.finish.  At most WWN_SMALL runs: the lane adds them in order.  More: it sets its bit.
//   heavy   one wavefront per bin with more than WWN_SMALL runs: WWN_WAVE contiguous shares in order, merged pairwise, lower
//           share first; the default's term last.
//
// SMOOTH, width w, h = w / 2.  The output is one run [p, p + 1) per position; a segment is one island.  With s = the first
// start and F = the last finish of the segment:
//   p0 = max(1, s - h); the positions read are q0 .. F - 1, q0 = 1 when s - h < 1 (the prefill reads 1 .. h first), else s.
//   Reading goes on while p + h <= F - 1, i.e. up to Pr = max(F - 1 - h, p0 - 1); from then on every pop drops the oldest value.
//   The window of output p is the positions [L(p), R(p)]:
//     R(p) = min(p + h, F - 1)
//     L(p) = max(p + h - w + 1, q0)                      p <= Pr
//            max(p + h - w + 1, q0 + (p - Pr - 1))       p >  Pr   (a chromosome shorter than w shrinks from its first read
//                                                                  position, one per pop, not by the window formula)
//   and the island ends with the last p whose window is not empty.  A position inside the segment that no run covers reads as
//   0 (NOT the default).  value(p) = (sum of the window) / w; NaN exactly while the window holds a NaN position.
//   ends    the first start and the last finish of every segment; the host lays out the islands, the clip and the strips
//   smooth  the work item is a STRIP of WWN_STRIP consecutive outputs, aligned to the segment's p0 (so the bits of a position
//           do not depend on the clip [clip_lo, clip_hi) of what is delivered, nor on the other segments): the first window
//           of the strip is summed from the runs under it as len * value in run order; the following windows slide with two
//           run cursors, + the value that enters, - the value that leaves.  The NaN positions of the window are COUNTED apart
//           from the sum.  A workgroup's 256 strips pass through LDS so that the 16 bytes per position leave coalesced.
//
// The bits of either result depend only on the segment's runs, the width and the default.
#ifndef WT_WINDOW_H_
#define WT_WINDOW_H_

#include <math.h>

#include "wt_cover.h"

#define WWN_BLOCK WCV_BLOCK
#define WWN_RUNS_PER_LANE 8                     // runs one lane of the count / cum passes takes
#define WWN_RUNS (WWN_BLOCK * WWN_RUNS_PER_LANE)
#define WWN_TILE 256                            // output bins of one workgroup of the bins pass: one per lane
#define WWN_SMALL 32                            // runs under a bin its own lane finishes
#define WWN_WAVE 64                             // shares of a wave-regime bin
#define WWN_WAVES (WWN_BLOCK / WWN_WAVE)
#define WWN_WINDOW 2048                         // scanned counts a workgroup stages in LDS (16 KiB)
#define WWN_STRIP 16                            // consecutive outputs one lane of the smooth pass slides over
#define WWN_STRIP_PAD (WWN_STRIP + 1)           // (odd: the lanes' strips start in different LDS banks)
#define WWN_POS (WWN_BLOCK * WWN_STRIP)         // outputs of one workgroup of the smooth pass

enum { WWN_OP_BIN = 0, WWN_OP_SMOOTH = 1 };
enum { WWN_K_VALID = 0, WWN_K_COUNT, WWN_K_CUM, WWN_K_BINS, WWN_K_HEAVY, WWN_K_ENDS, WWN_K_SMOOTH, WWN_K_COUNT_ };
enum { WWN_S_ERR = 0 /* runs that break the input rules */, WWN_S_RANGE = 1 /* bins past INT32_MAX */, WWN_S_NOUT = 2, WWN_S_NHEAVY = 3, WWN_S_N = 8 };

struct WwnHeavyLds {
    double part[WWN_BLOCK];
    long long cov[WWN_BLOCK];
};

struct WwnLds {
    union {
        long long ll[WWN_BLOCK];                    // count, cum: the lanes' sums
        long long win[WWN_WINDOW];                  // bins: the staged scanned counts
        WwnHeavyLds hv;                             // heavy: the lanes' shares
        double val[WWN_BLOCK * WWN_STRIP_PAD];      // smooth: the strips' values
    };
    unsigned int flag[WWN_BLOCK];                   // bins: 1: a wave-regime bin
    long long item[WWN_WAVES];                      // heavy: the wave's output bin, -1: none
    unsigned int cnt[WWN_WAVES];
    long long lo, hi;                               // bins: the runs of the tile
};

// one island of smooth (host-made, one per segment + a sentinel that only holds tile0)
struct WwnSeg {
    long long r0, r1;               // its runs
    long long p0, q0, F, Pr, pend;  // first output, first position read, last finish, last reading output, last output
    long long a, b;                 // outputs delivered: [a, b), inside [p0, pend + 1) and the clip
    long long out;                  // output index of a
    long long tile0, t0;            // the first workgroup of the island; the tile of the island it takes
};

struct WwnArgs {
    int op;
    const int32_t *start, *finish;
    const void *value;
    int value_is_f64;
    const int64_t *seg_off;         // [n_seg + 1]
    long long n_seg, n;
    long long width;
    double default_value;
    long long *scalars;             // [WWN_S_N]
    long long *blk;                 // [workgroups of count] their owned bins, then the bins before the workgroup
    long long *cum;                 // [n] output bins before the bins run i owns
    long long total;                // output bins
    int64_t *o_seg;                 // [n_seg + 1] device copy of the output offsets (bin)
    int32_t *o_start, *o_finish;
    double *o_value;
    unsigned long long *hmask;      // [4 per workgroup of bins] its wave-regime bins
    long long *hcnt;                // [workgroups of bins] their number, then the number before the workgroup
    long long hblocks, n_heavy;
    int32_t *ends;                  // [2 n_seg] first start, last finish (smooth)
    const WwnSeg *seg;              // [n_seg + 1]
};

WCV_DEV double wwn_value(const WwnArgs &a, long long i) {
    return a.value_is_f64 ? ((const double *) a.value)[i] : (double) ((const float *) a.value)[i];
}

// the grid bin of position p >= 1 (32-bit division: p - 1 and the width are below 2^31)
WCV_DEV long long wwn_bin_of(const WwnArgs &a, long long p) { return (long long) ((unsigned int) (p - 1) / (unsigned int) a.width); }

// the first bin run i owns; its last is the bin of finish - 1
WCV_DEV long long wwn_first_bin(const WwnArgs &a, long long i, long long g) {
    const long long fb = wwn_bin_of(a, a.start[i]);
    if (i == (long long) a.seg_off[g]) return fb;
    const long long pb = wwn_bin_of(a, (long long) a.finish[i - 1] - 1) + 1;
    return fb > pb ? fb : pb;
}

WCV_DEV long long wwn_owned(const WwnArgs &a, long long i) {
    return wwn_bin_of(a, (long long) a.finish[i] - 1) - wwn_first_bin(a, i, wcv_seg_of(a.seg_off, a.n_seg, i)) + 1;
}

// ---- valid: one lane per run ----
WCV_DEV void wwn_valid_block(const WwnArgs &a, long long block, WwnLds *) {
    WCV_LANES(l) {
        const long long i = block * WWN_BLOCK + l;
        if (i >= a.n) continue;
        const long long g = wcv_seg_of(a.seg_off, a.n_seg, i);
        const long long s = a.start[i], f = a.finish[i];
        bool bad = s >= f || s < 1;
        if (i > (long long) a.seg_off[g] && (long long) a.finish[i - 1] > s) bad = true;      // (with start < finish: sorted and disjoint)
        if (bad) wcv_add64(&a.scalars[WWN_S_ERR], 1);
        else if (a.op == WWN_OP_BIN && (wwn_bin_of(a, f - 1) + 1) * a.width + 1 > (long long) INT32_MAX) wcv_add64(&a.scalars[WWN_S_RANGE], 1);
    }
}

// ---- count: the bins the workgroup's runs own ----
WCV_DEV void wwn_count_block(const WwnArgs &a, long long block, WwnLds *lds) {
    WCV_LANES(l) {
        long long acc = 0;
        for (int k = 0; k < WWN_RUNS_PER_LANE; k++) {
            const long long i = block * WWN_RUNS + (long long) l * WWN_RUNS_PER_LANE + k;
            if (i < a.n) acc += wwn_owned(a, i);
        }
        lds->ll[l] = acc;
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (l == 0) {
            long long run = 0;
            for (int k = 0; k < WWN_BLOCK; k++) run += lds->ll[k];
            a.blk[block] = run;
        }
    }
}

// ---- cum: the exclusive scan per run (blk scanned); a segment's first run stores the segment's output offset ----
WCV_DEV void wwn_cum_block(const WwnArgs &a, long long block, WwnLds *lds) {
    WCV_LANES(l) {
        long long acc = 0;
        for (int k = 0; k < WWN_RUNS_PER_LANE; k++) {
            const long long i = block * WWN_RUNS + (long long) l * WWN_RUNS_PER_LANE + k;
            if (i < a.n) acc += wwn_owned(a, i);
        }
        lds->ll[l] = acc;
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (l == 0) {
            long long run = a.blk[block];
            for (int k = 0; k < WWN_BLOCK; k++) { const long long c = lds->ll[k]; lds->ll[k] = run; run += c; }
        }
    }
    WCV_SYNC();
    WCV_LANES(l) {
        long long run = lds->ll[l];
        for (int k = 0; k < WWN_RUNS_PER_LANE; k++) {
            const long long i = block * WWN_RUNS + (long long) l * WWN_RUNS_PER_LANE + k;
            if (i >= a.n) break;
            const long long g = wcv_seg_of(a.seg_off, a.n_seg, i);
            a.cum[i] = run;
            if (i == (long long) a.seg_off[g]) a.o_seg[g] = (int64_t) run;
            run += wwn_owned(a, i);
        }
    }
}

// the last k in [lo, hi) with cum[k] <= o (cum[lo] <= o)
WCV_DEV long long wwn_find(const long long *cum, long long lo, long long hi, long long o) {
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (cum[mid] <= o) lo = mid; else hi = mid;
    }
    return lo;
}

struct WwnBin {
    long long i, k1;                // the runs under the bin: [i, k1), i its owner
    long long bs, bf;               // the bin
};

// output bin o, owned by run i
WCV_DEV WwnBin wwn_bin(const WwnArgs &a, long long i, long long o) {
    WwnBin b;
    const long long g = wcv_seg_of(a.seg_off, a.n_seg, i);
    b.i = i;
    b.bs = 1 + (wwn_first_bin(a, i, g) + (o - a.cum[i])) * a.width;
    b.bf = b.bs + a.width;
    // the first run after the owner with start >= bf: a gallop from the owner (a bin seldom holds many runs), then a binary
    // search inside the last stride.  Runs before q0 start below bf; q1 is the segment's end or starts at bf or above.
    long long q0 = i + 1, q1 = (long long) a.seg_off[g + 1];
    for (long long step = 1; q0 < q1; step <<= 1) {
        const long long probe = q0 + step - 1 < q1 ? q0 + step - 1 : q1 - 1;
        if ((long long) a.start[probe] >= b.bf) { q1 = probe; break; }
        q0 = probe + 1;
    }
    while (q0 < q1) { const long long mid = (q0 + q1) >> 1; if ((long long) a.start[mid] >= b.bf) q1 = mid; else q0 = mid + 1; }
    b.k1 = q0;
    return b;
}

// share t of n: a contiguous stretch of the bin's runs, in order
WCV_DEV void wwn_share(const WwnArgs &a, const WwnBin &b, int t, int n, double *acc, long long *cov) {
    const long long nr = b.k1 - b.i, per = (nr + n - 1) / n;
    long long e0 = b.i + (long long) t * per, e1 = e0 + per;
    if (e1 > b.k1) e1 = b.k1;
    double x = 0.0;
    long long c = 0;
    for (long long k = e0; k < e1; k++) {
        long long u = a.start[k], w = a.finish[k];
        if (u < b.bs) u = b.bs;
        if (w > b.bf) w = b.bf;
        x += (double) (w - u) * wwn_value(a, k);
        c += w - u;
    }
    *acc = x; *cov = c;
}

// :1023-1024
WCV_DEV double wwn_with_default(const WwnArgs &a, double acc, long long cov) {
    const double d = a.default_value;
    if (d != 0.0 && cov < a.width) acc += (double) (a.width - cov) * d;        // (NaN != 0.0: true, as in C)
    return acc;
}

WCV_DEV bool wwn_is_heavy(const WwnBin &b) { return b.k1 - b.i > WWN_SMALL; }

// ---- bins: lane l of workgroup b has output bin 256 b + l ----
WCV_DEV void wwn_bins_block(const WwnArgs &a, long long block, WwnLds *lds) {
    const long long o0 = block * WWN_TILE, o1 = (o0 + WWN_TILE < a.total ? o0 + WWN_TILE : a.total) - 1;
    WCV_LANES(l) {
        if (l == 0) {
            lds->lo = wwn_find(a.cum, 0, a.n, o0);
            lds->hi = wwn_find(a.cum, lds->lo, a.n, o1) + 1;
        }
    }
    WCV_SYNC();
    WCV_LANES(l) {
        const long long lo = lds->lo, cnt = lds->hi - lo;
        if (cnt <= WWN_WINDOW)
            for (long long k = l; k < cnt; k += WWN_BLOCK) lds->win[k] = a.cum[lo + k];
    }
    WCV_SYNC();
    WCV_LANES(l) {
        const long long o = o0 + l, lo = lds->lo, hi = lds->hi;
        unsigned int heavy = 0;
        if (o <= o1) {
            const long long i = hi - lo <= WWN_WINDOW ? lo + wwn_find(lds->win, 0, hi - lo, o) : wwn_find(a.cum, lo, hi, o);
            const WwnBin b = wwn_bin(a, i, o);
            a.o_start[o] = (int32_t) b.bs;
            a.o_finish[o] = (int32_t) b.bf;
            if (wwn_is_heavy(b)) heavy = 1;
            else {
                double acc;
                long long cov;
                wwn_share(a, b, 0, 1, &acc, &cov);
                a.o_value[o] = wwn_with_default(a, acc, cov);
            }
        }
        lds->flag[l] = heavy;
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (l < WWN_WAVES) {
            unsigned long long m = 0;
            for (int k = 0; k < WWN_WAVE; k++) if (lds->flag[l * WWN_WAVE + k]) m |= 1ull << k;
            a.hmask[block * WWN_WAVES + l] = m;
            lds->cnt[l] = (unsigned int) wcv_popc(m);
        }
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (l == 0) {
            long long n = 0;
            for (int k = 0; k < WWN_WAVES; k++) n += lds->cnt[k];
            a.hcnt[block] = n;
        }
    }
}

// wave-regime bin q of the call (hcnt scanned) -> its output bin
WCV_DEV long long wwn_locate(const WwnArgs &a, long long q) {
    const long long b0 = wwn_find(a.hcnt, 0, a.hblocks, q);
    long long left = q - a.hcnt[b0];
    for (int w = 0; w < WWN_WAVES; w++) {
        const unsigned long long m = a.hmask[b0 * WWN_WAVES + w];
        const int c = wcv_popc(m);
        if (left >= c) { left -= c; continue; }
        for (int k = 0; k < WWN_WAVE; k++)
            if ((m >> k) & 1ull) { if (left == 0) return b0 * WWN_TILE + w * WWN_WAVE + k; left--; }
    }
    return -1;
}

// ---- heavy: wave w of workgroup b sums wave-regime bin 4 b + w ----
WCV_DEV void wwn_heavy_block(const WwnArgs &a, long long block, WwnLds *lds) {
    WCV_LANES(l) {
        const int w = l / WWN_WAVE, t = l % WWN_WAVE;
        const long long q = block * WWN_WAVES + w;
        double acc = 0.0;
        long long cov = 0, o = -1;
        if (q < a.n_heavy) o = wwn_locate(a, q);
        if (o >= 0) wwn_share(a, wwn_bin(a, wwn_find(a.cum, 0, a.n, o), o), t, WWN_WAVE, &acc, &cov);
        lds->hv.part[l] = acc;
        lds->hv.cov[l] = cov;
        if (t == 0) lds->item[w] = o;
    }
    for (int s = 1; s < WWN_WAVE; s <<= 1) {
        WCV_SYNC();
        WCV_LANES(l) {
            if ((l & (2 * s - 1)) == 0) { lds->hv.part[l] += lds->hv.part[l + s]; lds->hv.cov[l] += lds->hv.cov[l + s]; }
        }
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (l % WWN_WAVE == 0 && lds->item[l / WWN_WAVE] >= 0) a.o_value[lds->item[l / WWN_WAVE]] = wwn_with_default(a, lds->hv.part[l], lds->hv.cov[l]);
    }
}

// ---- ends: one lane per segment ----
WCV_DEV void wwn_ends_block(const WwnArgs &a, long long block, WwnLds *) {
    WCV_LANES(l) {
        const long long g = block * WWN_BLOCK + l;
        if (g >= a.n_seg) continue;
        const long long r0 = a.seg_off[g], r1 = a.seg_off[g + 1];
        a.ends[2 * g] = r1 > r0 ? a.start[r0] : 0;
        a.ends[2 * g + 1] = r1 > r0 ? a.finish[r1 - 1] : 0;
    }
}

// ---- smooth ----
WCV_DEV long long wwn_win_lo(const WwnSeg &s, long long w, long long p) {
    const long long x = p + w / 2 - w + 1, y = p <= s.Pr ? s.q0 : s.q0 + (p - s.Pr - 1);
    return x > y ? x : y;
}
WCV_DEV long long wwn_win_hi(const WwnSeg &s, long long w, long long p) {
    const long long x = p + w / 2;
    return x < s.F - 1 ? x : s.F - 1;
}

// The island of a segment: what the reference's loop (:1102-1136) comes to, see the head of this file.  first / last: the
// segment's first start (>= 1) and last finish; the clip [clip_lo, clip_hi), 0, 0: none.
static inline WwnSeg wwn_island(long long r0, long long r1, long long first, long long last, long long w, long long clip_lo, long long clip_hi) {
    WwnSeg s = {};
    const long long h = w / 2;
    s.r0 = r0; s.r1 = r1;
    s.F = last;
    s.p0 = first - h < 1 ? 1 : first - h;
    s.q0 = first - h < 1 ? 1 : first;
    s.Pr = last - 1 - h > s.p0 - 1 ? last - 1 - h : s.p0 - 1;
    const long long e1 = last - 2 - h + w, e2 = last - s.q0 + s.Pr;      // the last p with L(p) <= F - 1, either branch of the maximum
    s.pend = e1 < e2 ? e1 : e2;
    s.a = s.p0; s.b = s.pend + 1;
    if (clip_lo != 0 || clip_hi != 0) {
        if (clip_lo > s.a) s.a = clip_lo;
        if (clip_hi < s.b) s.b = clip_hi;
    }
    if (s.b < s.a) s.b = s.a;
    return s;
}

// the workgroups an island needs: the tiles of WWN_POS outputs, counted from p0, that meet [a, b)
static inline long long wwn_island_tiles(WwnSeg *s) {
    if (s->b <= s->a) { s->t0 = 0; return 0; }
    s->t0 = (s->a - s->p0) / WWN_POS;
    return (s->b - 1 - s->p0) / WWN_POS - s->t0 + 1;
}

WCV_DEV WwnSeg wwn_seg_of_tile(const WwnArgs &a, long long block) {
    long long g0 = 0, g1 = a.n_seg;                 // seg[g0].tile0 <= block < seg[g1].tile0
    while (g1 - g0 > 1) { const long long mid = (g0 + g1) >> 1; if (a.seg[mid].tile0 <= block) g0 = mid; else g1 = mid; }
    return a.seg[g0];
}

WCV_DEV void wwn_smooth_block(const WwnArgs &a, long long block, WwnLds *lds) {
    const long long w = a.width;
    WCV_LANES(l) {
        const WwnSeg s = wwn_seg_of_tile(a, block);
        const long long x0 = s.p0 + (s.t0 + block - s.tile0) * WWN_POS + (long long) l * WWN_STRIP;
        if (x0 >= s.b || x0 + WWN_STRIP <= s.a) continue;
        long long lo = wwn_win_lo(s, w, x0), hi = wwn_win_hi(s, w, x0);
        long long co = s.r0, q1 = s.r1;             // the first run with finish > lo
        while (co < q1) { const long long mid = (co + q1) >> 1; if ((long long) a.finish[mid] > lo) q1 = mid; else co = mid + 1; }
        double sum = 0.0;
        long long nan = 0, c = co;
        for (; c < s.r1 && (long long) a.start[c] <= hi; c++) {
            long long u = a.start[c], x = a.finish[c];
            if (u < lo) u = lo;
            if (x > hi + 1) x = hi + 1;
            const double v = wwn_value(a, c);
            if (v != v) nan += x - u; else sum += (double) (x - u) * v;
        }
        long long ci = c > co ? c - 1 : co;         // no run before it ends after hi
        for (int k = 0; k < WWN_STRIP; k++) {
            const long long p = x0 + k;
            if (p >= s.b) break;
            lds->val[l * WWN_STRIP_PAD + k] = nan > 0 ? (double) NAN : sum / (double) w;
            const long long nlo = wwn_win_lo(s, w, p + 1), nhi = wwn_win_hi(s, w, p + 1);
            if (nhi > hi) {                         // position nhi = hi + 1 enters
                while (ci < s.r1 && (long long) a.finish[ci] <= nhi) ci++;
                if (ci < s.r1 && (long long) a.start[ci] <= nhi) {
                    const double v = wwn_value(a, ci);
                    if (v != v) nan++; else sum += v;
                }
                hi = nhi;
            }
            if (nlo > lo) {                         // position lo leaves
                while (co < s.r1 && (long long) a.finish[co] <= lo) co++;
                if (co < s.r1 && (long long) a.start[co] <= lo) {
                    const double v = wwn_value(a, co);
                    if (v != v) nan--; else sum -= v;
                }
                lo = nlo;
            }
        }
    }
    WCV_SYNC();
    WCV_LANES(l) {
        const WwnSeg s = wwn_seg_of_tile(a, block);
        const long long xt = s.p0 + (s.t0 + block - s.tile0) * WWN_POS;
        for (int it = 0; it < WWN_STRIP; it++) {
            const int j = it * WWN_BLOCK + l;
            const long long p = xt + j;
            if (p < s.a || p >= s.b) continue;
            const long long o = s.out + (p - s.a);
            a.o_start[o] = (int32_t) p;
            a.o_finish[o] = (int32_t) (p + 1);
            a.o_value[o] = lds->val[(j / WWN_STRIP) * WWN_STRIP_PAD + j % WWN_STRIP];
        }
    }
}

WCV_DEV void wwn_run_block(int kernel, const WwnArgs &a, long long block, WwnLds *lds) {
    switch (kernel) {
    case WWN_K_VALID: wwn_valid_block(a, block, lds); break;
    case WWN_K_COUNT: wwn_count_block(a, block, lds); break;
    case WWN_K_CUM: wwn_cum_block(a, block, lds); break;
    case WWN_K_BINS: wwn_bins_block(a, block, lds); break;
    case WWN_K_HEAVY: wwn_heavy_block(a, block, lds); break;
    case WWN_K_ENDS: wwn_ends_block(a, block, lds); break;
    case WWN_K_SMOOTH: wwn_smooth_block(a, block, lds); break;
    default: break;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The two doors, written once over a Launcher: the one of wt_cover.h (alloc, release, zero, to_host, to_device, run over
// WcvArgs) with    bool run_window(int kernel, long long blocks, const WwnArgs &a)     and     bool sync()
// Return value: 0 fine, 1 bad argument, 2 launcher failure, 3 capacity (*n_out holds the count needed).  Nothing is written to
// the output arrays unless the value is 0.
// ---------------------------------------------------------------------------------------------------------------------
#ifndef WCV_NO_HOST

// what both doors open with: the argument checks, the offsets on the device, the validation pass.  n == 0 returns -1.
template <class L>
static int wwn_open(L &l, WcvScope<L> &sc, WwnArgs &a, const int64_t *seg_off, long long capacity, const int32_t *o_start, const int32_t *o_finish,
                    const double *o_value, int64_t *o_seg_off, int64_t *n_out, const char **why) {
    *why = "";
    if (a.n_seg < 0 || !seg_off || !o_seg_off || !n_out || capacity < 0) { *why = "bad argument"; return 1; }
    if (a.width < 2 || a.width > (long long) INT32_MAX) { *why = "the width must be 2 or more"; return 1; }
    for (long long g = 0; g < a.n_seg; g++) if (seg_off[g + 1] < seg_off[g]) { *why = "segment offsets decrease"; return 1; }
    a.n = a.n_seg ? (long long) (seg_off[a.n_seg] - seg_off[0]) : 0;
    *n_out = 0;
    if (a.n == 0) { for (long long g = 0; g <= a.n_seg; g++) o_seg_off[g] = 0; return -1; }
    if (!a.start || !a.finish || !a.value || seg_off[0] != 0 || a.n >= (1ll << 31)) { *why = "bad argument"; return 1; }
    if (capacity > 0 && (!o_start || !o_finish || !o_value)) { *why = "bad argument"; return 1; }
    int64_t *d_seg = nullptr;
    if (!sc.get(&d_seg, (size_t) a.n_seg + 1) || !sc.get(&a.scalars, (size_t) WWN_S_N)) { *why = "device memory"; return 2; }
    a.seg_off = d_seg;
    if (!l.to_device(d_seg, seg_off, sizeof(int64_t) * ((size_t) a.n_seg + 1)) || !l.zero(a.scalars, sizeof(long long) * WWN_S_N)) { *why = "copy"; return 2; }
    long long h_sc[WWN_S_N];
    if (!l.run_window(WWN_K_VALID, wcv_blocks(a.n, WWN_BLOCK), a) || !l.to_host(h_sc, a.scalars, sizeof h_sc)) { *why = "validation pass"; return 2; }
    if (h_sc[WWN_S_ERR]) { *why = "a segment is not sorted, holds a run with start >= finish or start < 1, or runs that overlap"; return 1; }
    if (h_sc[WWN_S_RANGE]) { *why = "an output coordinate would pass INT32_MAX"; return 1; }
    return 0;
}

// wtamd_runs_bin
template <class L>
static int wwn_bin_door(L &l, long long n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish, const void *value, int value_is_f64,
                        long long width, double default_value, long long capacity, int32_t *o_start, int32_t *o_finish, double *o_value,
                        int64_t *o_seg_off, int64_t *n_out, const char **why) {
    WwnArgs a = {};
    a.op = WWN_OP_BIN;
    a.start = start; a.finish = finish; a.value = value; a.value_is_f64 = value_is_f64;
    a.n_seg = n_seg; a.width = width; a.default_value = default_value;
    a.o_start = o_start; a.o_finish = o_finish; a.o_value = o_value;
    WcvScope<L> sc(l);
    if (const int rc = wwn_open(l, sc, a, seg_off, capacity, o_start, o_finish, o_value, o_seg_off, n_out, why)) return rc < 0 ? 0 : rc;
    const long long rblocks = wcv_blocks(a.n, WWN_RUNS);
    if (!sc.get(&a.blk, (size_t) rblocks) || !sc.get(&a.cum, (size_t) a.n) || !sc.get(&a.o_seg, (size_t) n_seg + 1)) { *why = "device memory"; return 2; }
    WcvArgs s = {};
    s.scan = a.blk; s.scan_n = rblocks; s.scan_init = nullptr; s.scan_total = &a.scalars[WWN_S_NOUT];
    long long h_sc[WWN_S_N];
    std::vector<int64_t> h_oseg((size_t) n_seg + 1);
    if (!l.zero(a.o_seg, sizeof(int64_t) * ((size_t) n_seg + 1)) || !l.run_window(WWN_K_COUNT, rblocks, a) || !l.run(WCV_K_SCAN_SUM, 1, s) ||
        !l.run_window(WWN_K_CUM, rblocks, a) || !l.to_host(h_sc, a.scalars, sizeof h_sc) || !l.to_host(h_oseg.data(), a.o_seg, sizeof(int64_t) * h_oseg.size()))
        { *why = "count passes"; return 2; }
    a.total = h_sc[WWN_S_NOUT];
    o_seg_off[n_seg] = a.total;
    for (long long q = n_seg - 1; q >= 0; q--) o_seg_off[q] = seg_off[q + 1] == seg_off[q] ? o_seg_off[q + 1] : h_oseg[(size_t) q];
    *n_out = a.total;
    if (a.total > capacity) return 3;
    a.hblocks = wcv_blocks(a.total, WWN_TILE);
    if (!sc.get(&a.hmask, (size_t) a.hblocks * WWN_WAVES) || !sc.get(&a.hcnt, (size_t) a.hblocks)) { *why = "device memory"; return 2; }
    s.scan = a.hcnt; s.scan_n = a.hblocks; s.scan_total = &a.scalars[WWN_S_NHEAVY];
    if (!l.run_window(WWN_K_BINS, a.hblocks, a) || !l.run(WCV_K_SCAN_SUM, 1, s) || !l.to_host(h_sc, a.scalars, sizeof h_sc)) { *why = "bins pass"; return 2; }
    a.n_heavy = h_sc[WWN_S_NHEAVY];
    if (!l.run_window(WWN_K_HEAVY, wcv_blocks(a.n_heavy, WWN_WAVES), a) || !l.sync()) { *why = "heavy pass"; return 2; }
    return 0;
}

// wtamd_runs_smooth
template <class L>
static int wwn_smooth_door(L &l, long long n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish, const void *value,
                           int value_is_f64, long long width, long long clip_lo, long long clip_hi, long long capacity, int32_t *o_start,
                           int32_t *o_finish, double *o_value, int64_t *o_seg_off, int64_t *n_out, const char **why) {
    WwnArgs a = {};
    a.op = WWN_OP_SMOOTH;
    a.start = start; a.finish = finish; a.value = value; a.value_is_f64 = value_is_f64;
    a.n_seg = n_seg; a.width = width;
    a.o_start = o_start; a.o_finish = o_finish; a.o_value = o_value;
    if (clip_lo < 0 || clip_hi < clip_lo) { *why = "the clip is not an interval"; return 1; }
    WcvScope<L> sc(l);
    if (const int rc = wwn_open(l, sc, a, seg_off, capacity, o_start, o_finish, o_value, o_seg_off, n_out, why)) return rc < 0 ? 0 : rc;
    WwnSeg *d_tab = nullptr;
    if (!sc.get(&a.ends, 2 * (size_t) n_seg) || !sc.get(&d_tab, (size_t) n_seg + 1)) { *why = "device memory"; return 2; }
    std::vector<int32_t> ends(2 * (size_t) n_seg);
    if (!l.run_window(WWN_K_ENDS, wcv_blocks(n_seg, WWN_BLOCK), a) || !l.to_host(ends.data(), a.ends, sizeof(int32_t) * ends.size())) { *why = "ends pass"; return 2; }
    std::vector<WwnSeg> tab((size_t) n_seg + 1);
    long long out = 0, tiles = 0;
    for (long long g = 0; g < n_seg; g++) {
        WwnSeg s = {};
        if (seg_off[g + 1] > seg_off[g]) {
            s = wwn_island(seg_off[g], seg_off[g + 1], ends[2 * (size_t) g], ends[2 * (size_t) g + 1], width, clip_lo, clip_hi);
            if (s.pend + 1 > (long long) INT32_MAX) { *why = "an output coordinate would pass INT32_MAX"; return 1; }
        }
        s.out = out; s.tile0 = tiles;
        o_seg_off[g] = out;
        out += s.b - s.a;
        tiles += wwn_island_tiles(&s);
        tab[(size_t) g] = s;
    }
    tab[(size_t) n_seg] = WwnSeg{};
    tab[(size_t) n_seg].tile0 = tiles; tab[(size_t) n_seg].out = out;
    o_seg_off[n_seg] = out;
    *n_out = out;
    if (out > capacity) return 3;
    a.seg = d_tab;
    if (!l.to_device(d_tab, tab.data(), sizeof(WwnSeg) * tab.size()) || !l.run_window(WWN_K_SMOOTH, tiles, a) || !l.sync()) { *why = "smooth pass"; return 2; }
    return 0;
}

#endif  // WCV_NO_HOST

// The same rules on the host, without a device (a translation unit compiled with -DWT_EMU: the passes above are then plain
// C++): one segment.  Bin: one forward sweep finds every output bin's owner, the bin itself is summed by the functions above,
// the wave regime's 64 shares one after the other, merged in the same order.  Smooth: the smooth pass itself, tile by tile.
// Return values as the doors'.
#ifdef WT_EMU
#include <vector>

static int wwn_host_check(long long n, const int32_t *start, const int32_t *finish, const double *value, long long width, long long capacity,
                          const int32_t *o_start, const int32_t *o_finish, const double *o_value, long long *n_out) {
    if (n < 0 || !n_out || capacity < 0 || width < 2 || width > (long long) INT32_MAX || n >= (1ll << 31) || (n > 0 && (!start || !finish || !value)) ||
        (capacity > 0 && (!o_start || !o_finish || !o_value)))
        return 1;
    for (long long i = 0; i < n; i++) if (start[i] < 1 || start[i] >= finish[i] || (i > 0 && finish[i - 1] > start[i])) return 1;
    return 0;
}

static int wwn_bin_host(long long n, const int32_t *start, const int32_t *finish, const double *value, long long width, double default_value,
                        long long capacity, int32_t *o_start, int32_t *o_finish, double *o_value, long long *n_out) {
    if (wwn_host_check(n, start, finish, value, width, capacity, o_start, o_finish, o_value, n_out)) return 1;
    *n_out = 0;
    if (n == 0) return 0;
    const int64_t seg[2] = {0, (int64_t) n};
    WwnArgs a = {};
    a.op = WWN_OP_BIN;
    a.start = start; a.finish = finish; a.value = value; a.value_is_f64 = 1;
    a.seg_off = seg; a.n_seg = 1; a.n = n; a.width = width; a.default_value = default_value;
    if ((wwn_bin_of(a, (long long) finish[n - 1] - 1) + 1) * width + 1 > (long long) INT32_MAX) return 1;
    std::vector<long long> cum((size_t) n);
    long long total = 0;
    for (long long i = 0; i < n; i++) { cum[(size_t) i] = total; total += wwn_owned(a, i); }
    a.cum = cum.data(); a.total = total;
    *n_out = total;
    if (total > capacity) return 3;
    long long i = 0;
    for (long long o = 0; o < total; o++) {
        while (i + 1 < n && cum[(size_t) i + 1] <= o) i++;
        const WwnBin b = wwn_bin(a, i, o);
        double acc;
        long long cov;
        if (!wwn_is_heavy(b)) wwn_share(a, b, 0, 1, &acc, &cov);
        else {
            double part[WWN_WAVE];
            long long pc[WWN_WAVE];
            for (int t = 0; t < WWN_WAVE; t++) wwn_share(a, b, t, WWN_WAVE, &part[t], &pc[t]);
            for (int s = 1; s < WWN_WAVE; s <<= 1)
                for (int t = 0; t < WWN_WAVE; t += 2 * s) { part[t] += part[t + s]; pc[t] += pc[t + s]; }
            acc = part[0]; cov = pc[0];
        }
        o_start[o] = (int32_t) b.bs; o_finish[o] = (int32_t) b.bf;
        o_value[o] = wwn_with_default(a, acc, cov);
    }
    return 0;
}

static int wwn_smooth_host(long long n, const int32_t *start, const int32_t *finish, const double *value, long long width, long long clip_lo,
                           long long clip_hi, long long capacity, int32_t *o_start, int32_t *o_finish, double *o_value, long long *n_out) {
    if (wwn_host_check(n, start, finish, value, width, capacity, o_start, o_finish, o_value, n_out) || clip_lo < 0 || clip_hi < clip_lo) return 1;
    *n_out = 0;
    if (n == 0) return 0;
    WwnSeg tab[2] = {};
    tab[0] = wwn_island(0, n, start[0], finish[n - 1], width, clip_lo, clip_hi);
    if (tab[0].pend + 1 > (long long) INT32_MAX) return 1;
    const long long tiles = wwn_island_tiles(&tab[0]);
    tab[1].tile0 = tiles;
    *n_out = tab[0].b - tab[0].a;
    if (*n_out > capacity) return 3;
    WwnArgs a = {};
    a.op = WWN_OP_SMOOTH;
    a.start = start; a.finish = finish; a.value = value; a.value_is_f64 = 1;
    a.n_seg = 1; a.n = n; a.width = width;
    a.o_start = o_start; a.o_finish = o_finish; a.o_value = o_value;
    a.seg = tab;
    std::vector<WwnLds> lds(1);
    for (long long t = 0; t < tiles; t++) wwn_smooth_block(a, t, lds.data());
    return 0;
}
#endif  // WT_EMU

#endif  // WT_WINDOW_H_
