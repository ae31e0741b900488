// wt_cover.h -- coverage and union of OVERLAPPING intervals (device + -DWT_EMU): the reference's CoverageWiggleIterator
// (src/unaryOps.c:303-375) and UnionWiggleIterator (:60-92) over whole run lists.  This header is the single source of the
// logic.  It is compiled
//   * by hipcc for gfx950 inside csrc/wt_cover.hip (the product), and
//   * by g++ with -DWT_EMU inside tests/cover_emu.cpp, which runs the workgroups of every pass one after the other in any
//     order on the CPU (the passes only meet through integer atomics and kernel boundaries, so the order cannot matter).
//
// Every pass is a function of (arguments, workgroup index): its lanes are written as WCV_LANES loops separated by
// WCV_SYNC -- one trip and __syncthreads() on the device, 256 trips and nothing under WT_EMU.  No pass waits for another
// workgroup: whatever crosses workgroups crosses a kernel boundary (two-level scans as three kernels).
//
// Input (the layout of wtamd_runs_map): n_seg segments, seg_off[n_seg + 1], start / finish; inside a segment the intervals
// are sorted by start and start < finish.  Coverage with WCV_ANY_ORDER takes a segment's intervals in any order (what the
// covering components of spliced reads are): only the pre-pass looks at the order -- its check, which the flag switches off;
// a segment's extent is the minimum of its starts and the maximum of its finishes, both by integer atomics; every other pass
// places an interval by its own start and finish alone, whole segments and pieces alike.
//
// COVERAGE of one segment.  B = the sorted distinct starts and finishes; run [B[k], B[k+1]) with value
// #(start <= B[k]) - #(finish <= B[k]) wherever that is > 0 (runs are NOT merged where the depth does not change, as the
// reference does not).
//   mark    one lane per interval sets the bits of its start and finish in a bitmap over the segment's positions
//   rank    popcounts of the bitmap words: per-word rank inside 2048-word blocks + block counts; scan of the block counts
//   delta   one lane per interval: +1 at the rank of its start, -1 at the rank of its finish (integer atomics), and the
//           position of either breakpoint into pos[rank]
//   depth   two-level inclusive scan of delta; count of the breakpoints with depth > 0; scan of the counts
//   emit    breakpoint k with depth > 0 -> run [pos[k], pos[k+1]) = depth
// Several segments share one bitmap (each from a word boundary): a segment's +1 / -1 sum to zero, so one scan over all of
// them gives every segment's depth.  A segment whose bitmap exceeds the scratch budget is cut at positions: the piece
// [c0, c1) takes the events inside it, starts its scan from the carry #(start < c0) - #(finish < c0), and a run still open at
// c1 gets its finish from the first breakpoint of a later piece.
//
// UNION of one segment: intervals join the current group while group.finish > start.  Inclusive prefix maximum over the keys
// (segment << 32 | finish); interval i leads a group iff it is the first of its segment or start[i] >= prefmax[i-1]; the
// group's finish is the prefix maximum at its last member.
#ifndef WT_COVER_H_
#define WT_COVER_H_

#include <stdint.h>

#define WCV_BLOCK 256
#define WCV_PER_LANE 8
#define WCV_TILE (WCV_BLOCK * WCV_PER_LANE)      // items (bitmap words, breakpoints, intervals) one workgroup ranks / scans
#define WCV_ANY_ORDER 1u                         // coverage flag (WTAMD_COVER_ANY_ORDER): a segment's intervals in any order

#ifdef WT_EMU
#define WCV_DEV inline
#define WCV_LANES(l) for (int l = 0; l < WCV_BLOCK; l++)
#define WCV_SYNC() do { } while (0)
WCV_DEV void wcv_or64(unsigned long long *p, unsigned long long v) { *p |= v; }
WCV_DEV void wcv_add32(int *p, int v) { *p += v; }
WCV_DEV void wcv_max32(int *p, int v) { if (v > *p) *p = v; }
WCV_DEV void wcv_min32(int *p, int v) { if (v < *p) *p = v; }
WCV_DEV void wcv_add64(long long *p, long long v) { *p += v; }
WCV_DEV int wcv_popc(unsigned long long x) { return __builtin_popcountll(x); }
#else
#include <hip/hip_runtime.h>
#define WCV_DEV __device__ __forceinline__
#define WCV_LANES(l) for (int l = (int) threadIdx.x, once_ = 1; once_; once_ = 0)
#define WCV_SYNC() __syncthreads()
WCV_DEV void wcv_or64(unsigned long long *p, unsigned long long v) { atomicOr(p, v); }
WCV_DEV void wcv_add32(int *p, int v) { atomicAdd(p, v); }
WCV_DEV void wcv_max32(int *p, int v) { atomicMax(p, v); }
WCV_DEV void wcv_min32(int *p, int v) { atomicMin(p, v); }
WCV_DEV void wcv_add64(long long *p, long long v) { atomicAdd((unsigned long long *) p, (unsigned long long) v); }
WCV_DEV int wcv_popc(unsigned long long x) { return __popcll(x); }
#endif

// scalars[] slots (device, 64-bit each)
enum { WCV_S_NBP = 0 /* breakpoints of the pass */, WCV_S_CARRY = 1 /* depth entering a piece */, WCV_S_NOUT = 2 /* runs the pass emits */,
       WCV_S_ERR = 3 /* != 0: unsorted starts or start >= finish */, WCV_S_LAST = 4 /* depth at the last breakpoint */, WCV_S_N = 8 };

enum { WCV_K_PRE = 0, WCV_K_MARK, WCV_K_RANK, WCV_K_SCAN_SUM, WCV_K_DELTA, WCV_K_DSUM, WCV_K_DEPTH, WCV_K_EMIT, WCV_K_SEGOFF,
       WCV_K_UKEY, WCV_K_SCAN_MAX, WCV_K_UPM, WCV_K_UHEAD, WCV_K_UEMIT, WCV_K_COUNT_ };

struct WcvLds {
    long long ll[WCV_BLOCK];
    unsigned int u[WCV_BLOCK];
    int acc;
    int same;
    int lo;
};

// One record for every pass (each reads what it needs); device pointers unless said otherwise.
struct WcvArgs {
    const int32_t *start, *finish;
    const int64_t *seg_off;         // [n_seg + 1]
    long long n_seg;
    long long i0, i1;               // intervals of the pass
    // per segment: the positions [wlo, whi) its bitmap holds and the bit it starts at (a multiple of 64)
    const long long *wlo, *whi, *bbase;
    int chunked;                    // the pass is one piece of one segment: events outside [wlo, whi) feed the carry
    unsigned long long *bits;
    long long n_words;
    unsigned int *wrank;            // [n_words] set bits before the word inside its 2048-word block
    long long *blk;                 // [word blocks] set bits before the block
    int32_t *delta;                 // [t_cap] +1 / -1 per breakpoint, then the depth
    int32_t *pos;                   // [t_cap] position of the breakpoint
    long long t_cap;
    long long *dblk, *pblk;         // [breakpoint blocks] depth before the block / emitted runs before the block
    long long *scalars;
    int32_t *segmax, *segmin;       // [n_seg] largest finish, smallest start (pre-pass)
    int any_order;                  // the pre-pass does not ask for starts in order
    // single-workgroup scans
    long long *scan;
    long long scan_n;
    const long long *scan_init;     // may be NULL (0)
    long long *scan_total;          // may be NULL
    // output
    int32_t *o_start, *o_finish;
    double *o_value;
    long long out_base, capacity;
    long long patch;                // >= 0: output run left open by an earlier piece; its finish is this pass's first breakpoint
    int64_t *o_seg;                 // [n_seg + 1] device copy of the output offsets
    long long seg_a, seg_b;         // segments of the pass
    // union
    const void *value;
    int value_is_f64;
    unsigned long long *pm;         // [n] inclusive prefix maximum of the keys
};

// the segment interval i lies in: the last g with seg_off[g] <= i (empty segments are skipped by construction)
WCV_DEV long long wcv_seg_of(const int64_t *seg_off, long long n_seg, long long i) {
    long long lo = 0, hi = n_seg;          // seg_off[lo] <= i < seg_off[hi]
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if ((long long) seg_off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- pre-pass: validation + the smallest start and the largest finish of every segment (one lane per interval) ----
WCV_DEV void wcv_pre_block(const WcvArgs &a, long long block, WcvLds *lds) {
    const long long b0 = a.i0 + block * WCV_BLOCK;
    const long long last = (b0 + WCV_BLOCK <= a.i1 ? b0 + WCV_BLOCK : a.i1) - 1;
    WCV_LANES(l) {
        if (l == 0) {
            lds->acc = INT32_MIN;
            lds->lo = INT32_MAX;
            // the whole workgroup in one segment (nearly always): one atomic per workgroup, not one per lane
            lds->same = wcv_seg_of(a.seg_off, a.n_seg, b0) == wcv_seg_of(a.seg_off, a.n_seg, last);
        }
    }
    WCV_SYNC();
    WCV_LANES(l) {
        const long long i = b0 + l;
        if (i >= a.i1) continue;
        const long long g = wcv_seg_of(a.seg_off, a.n_seg, i);
        const int32_t s = a.start[i], f = a.finish[i];
        bool bad = s >= f;
        if (!a.any_order && i > (long long) a.seg_off[g] && a.start[i - 1] > s) bad = true;
        if (bad) wcv_add64(&a.scalars[WCV_S_ERR], 1);
        if (lds->same) { wcv_max32(&lds->acc, f); wcv_min32(&lds->lo, s); }
        else { wcv_max32(&a.segmax[g], f); wcv_min32(&a.segmin[g], s); }
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (l == 0 && lds->same) {
            const long long g = wcv_seg_of(a.seg_off, a.n_seg, b0);
            wcv_max32(&a.segmax[g], lds->acc);
            wcv_min32(&a.segmin[g], lds->lo);
        }
    }
}

// ---- mark: one lane per interval, two bits ----
WCV_DEV void wcv_mark_block(const WcvArgs &a, long long block, WcvLds *) {
    WCV_LANES(l) {
        const long long i = a.i0 + block * WCV_BLOCK + l;
        if (i >= a.i1) continue;
        const long long g = wcv_seg_of(a.seg_off, a.n_seg, i);
        const long long lo = a.wlo[g], hi = a.whi[g], base = a.bbase[g];
        const long long s = a.start[i], f = a.finish[i];
        if (s >= lo && s < hi) { const long long b = base + (s - lo); wcv_or64(&a.bits[b >> 6], 1ull << (b & 63)); }
        if (f >= lo && f < hi) { const long long b = base + (f - lo); wcv_or64(&a.bits[b >> 6], 1ull << (b & 63)); }
    }
}

// ---- rank: per-word rank inside the block, block count ----
WCV_DEV void wcv_rank_block(const WcvArgs &a, long long block, WcvLds *lds) {
    const long long w0 = block * WCV_TILE;
    WCV_LANES(l) {
        unsigned int c = 0;
        for (int k = 0; k < WCV_PER_LANE; k++) {
            const long long w = w0 + (long long) l * WCV_PER_LANE + k;
            if (w < a.n_words) c += (unsigned) wcv_popc(a.bits[w]);
        }
        lds->u[l] = c;
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (l == 0) {
            unsigned int run = 0;
            for (int k = 0; k < WCV_BLOCK; k++) { const unsigned int c = lds->u[k]; lds->u[k] = run; run += c; }
            a.blk[block] = (long long) run;
        }
    }
    WCV_SYNC();
    WCV_LANES(l) {
        unsigned int run = lds->u[l];
        for (int k = 0; k < WCV_PER_LANE; k++) {
            const long long w = w0 + (long long) l * WCV_PER_LANE + k;
            if (w < a.n_words) { a.wrank[w] = run; run += (unsigned) wcv_popc(a.bits[w]); }
        }
    }
}

// ---- exclusive scan of scan[0 .. scan_n) by ONE workgroup: slices per lane, the 256 slice sums by lane 0 ----
template <bool MAX>
WCV_DEV void wcv_scan_block(const WcvArgs &a, long long block, WcvLds *lds) {
    if (block != 0) return;
    const long long per = (a.scan_n + WCV_BLOCK - 1) / WCV_BLOCK;
    unsigned long long *p = (unsigned long long *) a.scan;
    WCV_LANES(l) {
        const long long k0 = (long long) l * per, k1 = k0 + per < a.scan_n ? k0 + per : a.scan_n;
        unsigned long long acc = 0;
        for (long long k = k0; k < k1; k++) acc = MAX ? (p[k] > acc ? p[k] : acc) : acc + p[k];
        lds->ll[l] = (long long) acc;
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (l == 0) {
            unsigned long long run = a.scan_init ? (unsigned long long) *a.scan_init : 0ull;
            for (int k = 0; k < WCV_BLOCK; k++) {
                const unsigned long long c = (unsigned long long) lds->ll[k];
                lds->ll[k] = (long long) run;
                run = MAX ? (c > run ? c : run) : run + c;
            }
            if (a.scan_total) *a.scan_total = (long long) run;
        }
    }
    WCV_SYNC();
    WCV_LANES(l) {
        const long long k0 = (long long) l * per, k1 = k0 + per < a.scan_n ? k0 + per : a.scan_n;
        unsigned long long run = (unsigned long long) lds->ll[l];
        for (long long k = k0; k < k1; k++) {
            const unsigned long long c = p[k];
            p[k] = run;
            run = MAX ? (c > run ? c : run) : run + c;
        }
    }
}

// rank of bit b (which is set) among the set bits of the pass
WCV_DEV long long wcv_rank_of(const WcvArgs &a, long long b) {
    const long long w = b >> 6;
    const unsigned long long below = a.bits[w] & ((1ull << (b & 63)) - 1ull);
    return a.blk[w / WCV_TILE] + (long long) a.wrank[w] + wcv_popc(below);
}

// ---- delta: one lane per interval, +1 / -1 at the ranks of its breakpoints ----
WCV_DEV void wcv_delta_block(const WcvArgs &a, long long block, WcvLds *lds) {
    WCV_LANES(l) { if (l == 0) lds->acc = 0; }
    WCV_SYNC();
    WCV_LANES(l) {
        const long long i = a.i0 + block * WCV_BLOCK + l;
        if (i >= a.i1) continue;
        const long long g = wcv_seg_of(a.seg_off, a.n_seg, i);
        const long long lo = a.wlo[g], hi = a.whi[g], base = a.bbase[g];
        const long long s = a.start[i], f = a.finish[i];
        if (s >= lo && s < hi) {
            const long long r = wcv_rank_of(a, base + (s - lo));
            if (r < a.t_cap) { wcv_add32(&a.delta[r], 1); a.pos[r] = (int32_t) s; }      // (every writer of pos[r] writes the same value)
        }
        if (f >= lo && f < hi) {
            const long long r = wcv_rank_of(a, base + (f - lo));
            if (r < a.t_cap) { wcv_add32(&a.delta[r], -1); a.pos[r] = (int32_t) f; }
        }
        if (a.chunked) {
            const int c = (s < lo ? 1 : 0) - (f < lo ? 1 : 0);
            if (c) wcv_add32(&lds->acc, c);
        }
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (l == 0 && a.chunked && lds->acc) wcv_add64(&a.scalars[WCV_S_CARRY], (long long) lds->acc);
    }
}

// ---- depth, level 1: sum of the block's deltas ----
WCV_DEV void wcv_dsum_block(const WcvArgs &a, long long block, WcvLds *lds) {
    const long long T = a.scalars[WCV_S_NBP] < a.t_cap ? a.scalars[WCV_S_NBP] : a.t_cap;
    WCV_LANES(l) {
        long long acc = 0;
        for (int k = 0; k < WCV_PER_LANE; k++) {
            const long long r = block * WCV_TILE + (long long) l * WCV_PER_LANE + k;
            if (r < T) acc += a.delta[r];
        }
        lds->ll[l] = acc;
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (l == 0) {
            long long run = 0;
            for (int k = 0; k < WCV_BLOCK; k++) run += lds->ll[k];
            a.dblk[block] = run;
        }
    }
}

// ---- depth, level 2: inclusive scan inside the block (delta becomes the depth), count of the breakpoints with depth > 0 ----
WCV_DEV void wcv_depth_block(const WcvArgs &a, long long block, WcvLds *lds) {
    const long long T = a.scalars[WCV_S_NBP] < a.t_cap ? a.scalars[WCV_S_NBP] : a.t_cap;
    WCV_LANES(l) {
        long long acc = 0;
        for (int k = 0; k < WCV_PER_LANE; k++) {
            const long long r = block * WCV_TILE + (long long) l * WCV_PER_LANE + k;
            if (r < T) acc += a.delta[r];
        }
        lds->ll[l] = acc;
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (l == 0) {
            long long run = a.dblk[block];
            for (int k = 0; k < WCV_BLOCK; k++) { const long long c = lds->ll[k]; lds->ll[k] = run; run += c; }
        }
    }
    WCV_SYNC();
    WCV_LANES(l) {
        long long run = lds->ll[l];
        unsigned int cnt = 0;
        for (int k = 0; k < WCV_PER_LANE; k++) {
            const long long r = block * WCV_TILE + (long long) l * WCV_PER_LANE + k;
            if (r >= T) break;
            run += a.delta[r];
            a.delta[r] = (int32_t) run;
            if (run > 0) cnt++;
            if (r == T - 1) a.scalars[WCV_S_LAST] = run;
        }
        lds->u[l] = cnt;
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (l == 0) {
            long long run = 0;
            for (int k = 0; k < WCV_BLOCK; k++) run += lds->u[k];
            a.pblk[block] = run;
        }
    }
}

// ---- emit: breakpoint r with depth > 0 -> run [pos[r], pos[r+1]) ----
WCV_DEV void wcv_emit_block(const WcvArgs &a, long long block, WcvLds *lds) {
    const long long T = a.scalars[WCV_S_NBP] < a.t_cap ? a.scalars[WCV_S_NBP] : a.t_cap;
    WCV_LANES(l) {
        unsigned int cnt = 0;
        for (int k = 0; k < WCV_PER_LANE; k++) {
            const long long r = block * WCV_TILE + (long long) l * WCV_PER_LANE + k;
            if (r < T && a.delta[r] > 0) cnt++;
        }
        lds->u[l] = cnt;
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (l == 0) {
            long long run = a.pblk[block];
            for (int k = 0; k < WCV_BLOCK; k++) { const long long c = lds->u[k]; lds->ll[k] = run; run += c; }
        }
    }
    WCV_SYNC();
    WCV_LANES(l) {
        long long o = a.out_base + lds->ll[l];
        for (int k = 0; k < WCV_PER_LANE; k++) {
            const long long r = block * WCV_TILE + (long long) l * WCV_PER_LANE + k;
            if (r >= T) break;
            if (r == 0 && a.patch >= 0 && a.patch < a.capacity) a.o_finish[a.patch] = a.pos[0];
            const int32_t d = a.delta[r];
            if (d <= 0) continue;
            if (o < a.capacity) {
                a.o_start[o] = a.pos[r];
                a.o_finish[o] = r + 1 < T ? a.pos[r + 1] : INT32_MAX;      // (open at the end of a piece: patched by a later one)
                a.o_value[o] = (double) d;
            }
            o++;
        }
    }
}

// ---- output offset of every non-empty segment of the pass (one lane per segment) ----
WCV_DEV void wcv_segoff_block(const WcvArgs &a, long long block, WcvLds *) {
    WCV_LANES(l) {
        const long long g = a.seg_a + block * WCV_BLOCK + l;
        if (g >= a.seg_b || a.seg_off[g] == a.seg_off[g + 1]) continue;
        const long long w = a.bbase[g] >> 6;                                // the segment's smallest start is bit 0 of this word
        const long long r0 = a.blk[w / WCV_TILE] + (long long) a.wrank[w];
        const long long b = r0 / WCV_TILE;
        long long o = a.pblk[b];
        for (long long r = b * WCV_TILE; r < r0; r++) o += a.delta[r] > 0 ? 1 : 0;
        a.o_seg[g] = (int64_t) (a.out_base + o);
    }
}

// ---- union ----
WCV_DEV unsigned long long wcv_ukey(long long g, int32_t finish) {
    return ((unsigned long long) g << 32) | (unsigned long long) ((uint32_t) finish ^ 0x80000000u);
}
WCV_DEV int32_t wcv_ukey_finish(unsigned long long key) { return (int32_t) ((uint32_t) (key & 0xffffffffull) ^ 0x80000000u); }

// validation + the block's largest key
WCV_DEV void wcv_ukey_block(const WcvArgs &a, long long block, WcvLds *lds) {
    WCV_LANES(l) {
        unsigned long long m = 0;
        for (int k = 0; k < WCV_PER_LANE; k++) {
            const long long i = a.i0 + block * WCV_TILE + (long long) l * WCV_PER_LANE + k;
            if (i >= a.i1) break;
            const long long g = wcv_seg_of(a.seg_off, a.n_seg, i);
            const int32_t s = a.start[i], f = a.finish[i];
            bool bad = s >= f;
            if (i > (long long) a.seg_off[g] && a.start[i - 1] > s) bad = true;
            if (bad) wcv_add64(&a.scalars[WCV_S_ERR], 1);
            const unsigned long long key = wcv_ukey(g, f);
            if (key > m) m = key;
        }
        lds->ll[l] = (long long) m;
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (l == 0) {
            unsigned long long m = 0;
            for (int k = 0; k < WCV_BLOCK; k++) if ((unsigned long long) lds->ll[k] > m) m = (unsigned long long) lds->ll[k];
            a.scan[block] = (long long) m;          // (a.scan: the per-block maxima)
        }
    }
}

// inclusive prefix maximum inside the block, seeded with the maximum of everything before it
WCV_DEV void wcv_upm_block(const WcvArgs &a, long long block, WcvLds *lds) {
    WCV_LANES(l) {
        unsigned long long m = 0;
        for (int k = 0; k < WCV_PER_LANE; k++) {
            const long long i = a.i0 + block * WCV_TILE + (long long) l * WCV_PER_LANE + k;
            if (i >= a.i1) break;
            const unsigned long long key = wcv_ukey(wcv_seg_of(a.seg_off, a.n_seg, i), a.finish[i]);
            if (key > m) m = key;
        }
        lds->ll[l] = (long long) m;
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (l == 0) {
            unsigned long long run = (unsigned long long) a.scan[block];
            for (int k = 0; k < WCV_BLOCK; k++) {
                const unsigned long long c = (unsigned long long) lds->ll[k];
                lds->ll[k] = (long long) run;
                if (c > run) run = c;
            }
        }
    }
    WCV_SYNC();
    WCV_LANES(l) {
        unsigned long long run = (unsigned long long) lds->ll[l];
        for (int k = 0; k < WCV_PER_LANE; k++) {
            const long long i = a.i0 + block * WCV_TILE + (long long) l * WCV_PER_LANE + k;
            if (i >= a.i1) break;
            const unsigned long long key = wcv_ukey(wcv_seg_of(a.seg_off, a.n_seg, i), a.finish[i]);
            if (key > run) run = key;
            a.pm[i - a.i0] = run;
        }
    }
}

// interval i leads a group (pm complete)
WCV_DEV bool wcv_uhead(const WcvArgs &a, long long i) {
    if (i == a.i0) return true;
    const unsigned long long p = a.pm[i - 1 - a.i0];
    const long long g = wcv_seg_of(a.seg_off, a.n_seg, i);
    return (long long) (p >> 32) != g || a.start[i] >= wcv_ukey_finish(p);
}

WCV_DEV void wcv_uhead_block(const WcvArgs &a, long long block, WcvLds *lds) {
    WCV_LANES(l) {
        long long cnt = 0;
        for (int k = 0; k < WCV_PER_LANE; k++) {
            const long long i = a.i0 + block * WCV_TILE + (long long) l * WCV_PER_LANE + k;
            if (i >= a.i1) break;
            if (wcv_uhead(a, i)) cnt++;
        }
        lds->ll[l] = cnt;
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (l == 0) {
            long long run = 0;
            for (int k = 0; k < WCV_BLOCK; k++) run += lds->ll[k];
            a.pblk[block] = run;
        }
    }
}

// the leader writes start and value, the last member the finish; a segment's first interval its output offset
WCV_DEV void wcv_uemit_block(const WcvArgs &a, long long block, WcvLds *lds) {
    WCV_LANES(l) {
        long long cnt = 0;
        for (int k = 0; k < WCV_PER_LANE; k++) {
            const long long i = a.i0 + block * WCV_TILE + (long long) l * WCV_PER_LANE + k;
            if (i >= a.i1) break;
            if (wcv_uhead(a, i)) cnt++;
        }
        lds->u[l] = (unsigned int) cnt;
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (l == 0) {
            long long run = a.pblk[block];
            for (int k = 0; k < WCV_BLOCK; k++) { const long long c = lds->u[k]; lds->ll[k] = run; run += c; }
        }
    }
    WCV_SYNC();
    WCV_LANES(l) {
        long long heads = lds->ll[l];                   // leaders before interval i
        for (int k = 0; k < WCV_PER_LANE; k++) {
            const long long i = a.i0 + block * WCV_TILE + (long long) l * WCV_PER_LANE + k;
            if (i >= a.i1) break;
            const bool head = wcv_uhead(a, i);
            const bool tail = i + 1 >= a.i1 || wcv_uhead(a, i + 1);
            if (head) {
                const long long g = wcv_seg_of(a.seg_off, a.n_seg, i);
                if (i == (long long) a.seg_off[g]) a.o_seg[g] = (int64_t) heads;
                if (heads < a.capacity) {
                    a.o_start[heads] = a.start[i];
                    // bit for bit: a NaN keeps its payload, -0.0 its sign (f32 widens exactly)
                    if (a.o_value) {                                                    // (NULL: coordinates only, csrc/wt_region.h)
                        if (a.value_is_f64) ((unsigned long long *) a.o_value)[heads] = ((const unsigned long long *) a.value)[i];
                        else a.o_value[heads] = (double) ((const float *) a.value)[i];
                    }
                }
                heads++;
            }
            if (tail && heads - 1 < a.capacity) a.o_finish[heads - 1] = wcv_ukey_finish(a.pm[i - a.i0]);
        }
    }
}

WCV_DEV void wcv_run_block(int kernel, const WcvArgs &a, long long block, WcvLds *lds) {
    switch (kernel) {
    case WCV_K_PRE: wcv_pre_block(a, block, lds); break;
    case WCV_K_MARK: wcv_mark_block(a, block, lds); break;
    case WCV_K_RANK: wcv_rank_block(a, block, lds); break;
    case WCV_K_SCAN_SUM: wcv_scan_block<false>(a, block, lds); break;
    case WCV_K_DELTA: wcv_delta_block(a, block, lds); break;
    case WCV_K_DSUM: wcv_dsum_block(a, block, lds); break;
    case WCV_K_DEPTH: wcv_depth_block(a, block, lds); break;
    case WCV_K_EMIT: wcv_emit_block(a, block, lds); break;
    case WCV_K_SEGOFF: wcv_segoff_block(a, block, lds); break;
    case WCV_K_UKEY: wcv_ukey_block(a, block, lds); break;
    case WCV_K_SCAN_MAX: wcv_scan_block<true>(a, block, lds); break;
    case WCV_K_UPM: wcv_upm_block(a, block, lds); break;
    case WCV_K_UHEAD: wcv_uhead_block(a, block, lds); break;
    case WCV_K_UEMIT: wcv_uemit_block(a, block, lds); break;
    default: break;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The two doors, written once over a Launcher (the device: csrc/wt_runs_host.h; the CPU: tests/emu/runs_launcher.h):
//   void *alloc(size_t bytes)                 device memory, NULL on failure       void release(void *)
//   bool zero(void *p, size_t bytes)          bool to_host(void *h, const void *d, size_t)  (waits)
//   bool to_device(void *d, const void *h, size_t)
//   bool run(int kernel, long long blocks, const WcvArgs &a)
// Return value: 0 fine, 1 bad argument, 2 launcher failure, 3 capacity (the WTAMD_* codes).
// ---------------------------------------------------------------------------------------------------------------------
#ifndef WCV_NO_HOST
#include <vector>

static inline long long wcv_blocks(long long n, long long per) { return n > 0 ? (n + per - 1) / per : 0; }

template <class L>
struct WcvScope {            // frees what a door allocated, on every way out
    L &l;
    std::vector<void *> held;
    explicit WcvScope(L &l_) : l(l_) {}
    ~WcvScope() { for (void *p : held) l.release(p); }
    template <class T> bool get(T **p, size_t count) {
        *p = (T *) l.alloc(sizeof(T) * (count ? count : 1));
        if (*p) held.push_back((void *) *p);
        return *p != nullptr;
    }
    void drop_last(size_t k) { while (k-- && !held.empty()) { l.release(held.back()); held.pop_back(); } }
};

// coverage of one pass (several whole segments, or one piece of one segment): a.* describe it; returns the runs it emits
template <class L>
static int wcv_cover_pass(L &l, WcvArgs a, long long n_bits, long long *n_emitted, long long *last_depth, long long *n_bp) {
    WcvScope<L> sc(l);
    const long long n_iv = a.i1 - a.i0;
    a.n_words = (n_bits + 63) >> 6;
    const long long wblocks = wcv_blocks(a.n_words, WCV_TILE);
    a.t_cap = 2 * n_iv < a.n_words * 64 ? 2 * n_iv : a.n_words * 64;
    const long long tblocks = wcv_blocks(a.t_cap, WCV_TILE);
    if (!sc.get(&a.bits, (size_t) a.n_words) || !sc.get(&a.wrank, (size_t) a.n_words) || !sc.get(&a.blk, (size_t) wblocks) ||
        !sc.get(&a.delta, (size_t) a.t_cap) || !sc.get(&a.pos, (size_t) a.t_cap) || !sc.get(&a.dblk, (size_t) tblocks) ||
        !sc.get(&a.pblk, (size_t) tblocks) || !sc.get(&a.scalars, (size_t) WCV_S_N))
        return 2;
    if (!l.zero(a.bits, sizeof(unsigned long long) * (size_t) a.n_words) || !l.zero(a.delta, sizeof(int32_t) * (size_t) a.t_cap) ||
        !l.zero(a.scalars, sizeof(long long) * WCV_S_N))
        return 2;
    const long long iblocks = wcv_blocks(n_iv, WCV_BLOCK);
    bool ok = l.run(WCV_K_MARK, iblocks, a) && l.run(WCV_K_RANK, wblocks, a);
    WcvArgs s = a;
    s.scan = a.blk; s.scan_n = wblocks; s.scan_init = nullptr; s.scan_total = &a.scalars[WCV_S_NBP];
    ok = ok && l.run(WCV_K_SCAN_SUM, 1, s) && l.run(WCV_K_DELTA, iblocks, a) && l.run(WCV_K_DSUM, tblocks, a);
    s.scan = a.dblk; s.scan_n = tblocks; s.scan_init = &a.scalars[WCV_S_CARRY]; s.scan_total = nullptr;
    ok = ok && l.run(WCV_K_SCAN_SUM, 1, s) && l.run(WCV_K_DEPTH, tblocks, a);
    s.scan = a.pblk; s.scan_init = nullptr; s.scan_total = &a.scalars[WCV_S_NOUT];
    ok = ok && l.run(WCV_K_SCAN_SUM, 1, s) && l.run(WCV_K_EMIT, tblocks, a);
    if (ok && !a.chunked) ok = l.run(WCV_K_SEGOFF, wcv_blocks(a.seg_b - a.seg_a, WCV_BLOCK), a);
    long long h[WCV_S_N];
    if (!ok || !l.to_host(h, a.scalars, sizeof h)) return 2;
    *n_emitted = h[WCV_S_NOUT];
    *last_depth = h[WCV_S_LAST];
    *n_bp = h[WCV_S_NBP];
    return 0;
}

// wtamd_runs_coverage_flags.  budget: bytes of bitmap + word ranks (12 per 64 positions) one pass may hold.
template <class L>
static int wcv_coverage_flags(L &l, long long n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish, long long capacity,
                              int32_t *o_start, int32_t *o_finish, double *o_value, int64_t *o_seg_off, int64_t *n_out, long long budget,
                              unsigned int flags, const char **why) {
    *why = "";
    if (flags & ~WCV_ANY_ORDER) { *why = "unknown flag"; return 1; }
    if (n_seg < 0 || !seg_off || !o_seg_off || !n_out || capacity < 0) { *why = "bad argument"; return 1; }
    for (long long g = 0; g < n_seg; g++) if (seg_off[g + 1] < seg_off[g]) { *why = "segment offsets decrease"; return 1; }
    const long long n = n_seg ? (long long) (seg_off[n_seg] - seg_off[0]) : 0;
    *n_out = 0;
    if (n == 0) { for (long long g = 0; g <= n_seg; g++) o_seg_off[g] = 0; return 0; }
    if (!start || !finish || seg_off[0] != 0) { *why = "bad argument"; return 1; }
    WcvScope<L> sc(l);
    WcvArgs a = {};
    a.start = start; a.finish = finish; a.n_seg = n_seg; a.capacity = capacity;
    a.o_start = o_start; a.o_finish = o_finish; a.o_value = o_value; a.patch = -1;
    a.any_order = (flags & WCV_ANY_ORDER) != 0;
    int64_t *d_seg = nullptr;
    long long *d_tab = nullptr;
    if (!sc.get(&d_seg, (size_t) n_seg + 1) || !sc.get(&a.segmax, (size_t) n_seg) || !sc.get(&a.segmin, (size_t) n_seg) || !sc.get(&a.scalars, (size_t) WCV_S_N) ||
        !sc.get(&a.o_seg, (size_t) n_seg + 1) || !sc.get(&d_tab, (size_t) n_seg * 3))
        { *why = "device memory"; return 2; }
    a.seg_off = d_seg;
    std::vector<int32_t> h_max((size_t) n_seg, INT32_MIN), h_min((size_t) n_seg, INT32_MAX);
    if (!l.to_device(d_seg, seg_off, sizeof(int64_t) * ((size_t) n_seg + 1)) || !l.to_device(a.segmax, h_max.data(), sizeof(int32_t) * (size_t) n_seg) ||
        !l.to_device(a.segmin, h_min.data(), sizeof(int32_t) * (size_t) n_seg) ||
        !l.zero(a.scalars, sizeof(long long) * WCV_S_N) || !l.zero(a.o_seg, sizeof(int64_t) * ((size_t) n_seg + 1)))
        { *why = "copy"; return 2; }
    // pre-pass: validation, the extent of every segment
    a.i0 = 0; a.i1 = n;
    long long h_sc[WCV_S_N];
    if (!l.run(WCV_K_PRE, wcv_blocks(n, WCV_BLOCK), a) || !l.to_host(h_sc, a.scalars, sizeof h_sc) ||
        !l.to_host(h_max.data(), a.segmax, sizeof(int32_t) * (size_t) n_seg) || !l.to_host(h_min.data(), a.segmin, sizeof(int32_t) * (size_t) n_seg))
        { *why = "pre-pass"; return 2; }
    if (h_sc[WCV_S_ERR]) {
        *why = a.any_order ? "a segment holds an interval with start >= finish" : "a segment is not sorted by start, or holds an interval with start >= finish";
        return 1;
    }
    if ((capacity > 0 && (!o_start || !o_finish || !o_value))) { *why = "bad argument"; return 1; }
    const long long budget_words = budget / 12 > 1 ? budget / 12 : 1;
    std::vector<long long> tab((size_t) n_seg * 3, 0);      // wlo | whi | bbase
    a.wlo = d_tab; a.whi = d_tab + n_seg; a.bbase = d_tab + 2 * n_seg;
    long long out = 0;
    long long g = 0;
    while (g < n_seg) {
        if (seg_off[g + 1] == seg_off[g]) { g++; continue; }
        const long long lo = h_min[(size_t) g], hi = (long long) h_max[(size_t) g] + 1;      // positions [lo, hi)
        const long long words = (hi - lo + 63) >> 6;
        if (words > budget_words) {
            // one segment in pieces of budget_words * 64 positions
            o_seg_off[g] = out;
            a.chunked = 1; a.seg_a = g; a.seg_b = g + 1;
            a.i0 = seg_off[g]; a.i1 = seg_off[g + 1];
            a.patch = -1;
            for (long long c0 = lo; c0 < hi; c0 += budget_words * 64) {
                const long long c1 = c0 + budget_words * 64 < hi ? c0 + budget_words * 64 : hi;
                tab[(size_t) g] = c0; tab[(size_t) (n_seg + g)] = c1; tab[(size_t) (2 * n_seg + g)] = 0;
                if (!l.to_device(d_tab, tab.data(), sizeof(long long) * tab.size())) { *why = "copy"; return 2; }
                a.out_base = out;
                long long emitted = 0, last = 0, nbp = 0;
                if (wcv_cover_pass(l, a, c1 - c0, &emitted, &last, &nbp)) { *why = "coverage pass"; return 2; }
                if (nbp > 0) a.patch = last > 0 ? out + emitted - 1 : -1;
                out += emitted;
            }
            a.patch = -1;
            g++;
            continue;
        }
        // as many whole segments as the budget holds
        long long used = 0, e = g;
        while (e < n_seg) {
            if (seg_off[e + 1] == seg_off[e]) { e++; continue; }
            const long long w = ((long long) h_max[(size_t) e] + 1 - h_min[(size_t) e] + 63) >> 6;
            if (e > g && used + w > budget_words) break;
            if (w > budget_words) break;
            tab[(size_t) e] = h_min[(size_t) e]; tab[(size_t) (n_seg + e)] = (long long) h_max[(size_t) e] + 1; tab[(size_t) (2 * n_seg + e)] = used * 64;
            used += w;
            e++;
        }
        if (!l.to_device(d_tab, tab.data(), sizeof(long long) * tab.size())) { *why = "copy"; return 2; }
        a.chunked = 0; a.seg_a = g; a.seg_b = e; a.patch = -1;
        a.i0 = seg_off[g]; a.i1 = seg_off[e];
        a.out_base = out;
        long long emitted = 0, last = 0, nbp = 0;
        if (wcv_cover_pass(l, a, used * 64, &emitted, &last, &nbp)) { *why = "coverage pass"; return 2; }
        std::vector<int64_t> part((size_t) (e - g));
        if (!l.to_host(part.data(), a.o_seg + g, sizeof(int64_t) * part.size())) { *why = "copy"; return 2; }
        for (long long q = g; q < e; q++) o_seg_off[q] = part[(size_t) (q - g)];
        out += emitted;
        g = e;
    }
    o_seg_off[n_seg] = out;
    for (long long q = n_seg - 1; q >= 0; q--) if (seg_off[q + 1] == seg_off[q]) o_seg_off[q] = o_seg_off[q + 1];
    *n_out = out;
    return out > capacity ? 3 : 0;
}

// wtamd_runs_coverage: every segment sorted by start
template <class L>
static int wcv_coverage(L &l, long long n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish, long long capacity,
                        int32_t *o_start, int32_t *o_finish, double *o_value, int64_t *o_seg_off, int64_t *n_out, long long budget,
                        const char **why) {
    return wcv_coverage_flags(l, n_seg, seg_off, start, finish, capacity, o_start, o_finish, o_value, o_seg_off, n_out, budget, 0u, why);
}

// wtamd_runs_union
template <class L>
static int wcv_union(L &l, long long n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish, const void *value,
                     int value_is_f64, long long capacity, int32_t *o_start, int32_t *o_finish, double *o_value, int64_t *o_seg_off,
                     int64_t *n_out, const char **why) {
    *why = "";
    if (n_seg < 0 || !seg_off || !o_seg_off || !n_out || capacity < 0) { *why = "bad argument"; return 1; }
    for (long long g = 0; g < n_seg; g++) if (seg_off[g + 1] < seg_off[g]) { *why = "segment offsets decrease"; return 1; }
    const long long n = n_seg ? (long long) (seg_off[n_seg] - seg_off[0]) : 0;
    *n_out = 0;
    if (n == 0) { for (long long g = 0; g <= n_seg; g++) o_seg_off[g] = 0; return 0; }
    // (value and o_value both NULL: the groups' coordinates alone, what csrc/wt_region.h asks for a mask)
    if (!start || !finish || (!value && o_value) || seg_off[0] != 0 || n_seg >= (1ll << 31)) { *why = "bad argument"; return 1; }
    if ((capacity > 0 && (!o_start || !o_finish || (!o_value && value)))) { *why = "bad argument"; return 1; }
    WcvScope<L> sc(l);
    WcvArgs a = {};
    a.start = start; a.finish = finish; a.value = value; a.value_is_f64 = value_is_f64; a.n_seg = n_seg; a.capacity = capacity;
    a.o_start = o_start; a.o_finish = o_finish; a.o_value = o_value;
    a.i0 = 0; a.i1 = n;
    const long long blocks = wcv_blocks(n, WCV_TILE);
    int64_t *d_seg = nullptr;
    long long *d_bmax = nullptr;
    if (!sc.get(&d_seg, (size_t) n_seg + 1) || !sc.get(&a.scalars, (size_t) WCV_S_N) || !sc.get(&a.o_seg, (size_t) n_seg + 1) ||
        !sc.get(&d_bmax, (size_t) blocks) || !sc.get(&a.pblk, (size_t) blocks) || !sc.get(&a.pm, (size_t) n))
        { *why = "device memory"; return 2; }
    a.seg_off = d_seg;
    if (!l.to_device(d_seg, seg_off, sizeof(int64_t) * ((size_t) n_seg + 1)) || !l.zero(a.scalars, sizeof(long long) * WCV_S_N) ||
        !l.zero(a.o_seg, sizeof(int64_t) * ((size_t) n_seg + 1)))
        { *why = "copy"; return 2; }
    a.scan = d_bmax; a.scan_n = blocks;
    long long h_sc[WCV_S_N];
    if (!l.run(WCV_K_UKEY, blocks, a) || !l.to_host(h_sc, a.scalars, sizeof h_sc)) { *why = "key pass"; return 2; }
    if (h_sc[WCV_S_ERR]) { *why = "a segment is not sorted by start, or holds an interval with start >= finish"; return 1; }
    bool ok = l.run(WCV_K_SCAN_MAX, 1, a) && l.run(WCV_K_UPM, blocks, a) && l.run(WCV_K_UHEAD, blocks, a);
    WcvArgs s = a;
    s.scan = a.pblk; s.scan_total = &a.scalars[WCV_S_NOUT];
    ok = ok && l.run(WCV_K_SCAN_SUM, 1, s) && l.run(WCV_K_UEMIT, blocks, a);
    std::vector<int64_t> h_oseg((size_t) n_seg + 1);
    if (!ok || !l.to_host(h_sc, a.scalars, sizeof h_sc) || !l.to_host(h_oseg.data(), a.o_seg, sizeof(int64_t) * h_oseg.size()))
        { *why = "union passes"; return 2; }
    const long long out = h_sc[WCV_S_NOUT];
    o_seg_off[n_seg] = out;
    for (long long q = n_seg - 1; q >= 0; q--) o_seg_off[q] = seg_off[q + 1] == seg_off[q] ? o_seg_off[q + 1] : h_oseg[(size_t) q];
    *n_out = out;
    return out > capacity ? 3 : 0;
}
#endif  // WCV_NO_HOST

#endif  // WT_COVER_H_
