// wt_apply.h -- per-region statistics over whole run lists (device + -DWT_EMU): what the reference's ApplyMultiplexer
// (src/apply.c; the parser's `apply` / `apply_paste`, commandParser.c:266-320, 917-936) computes for every region of a BED
// file -- AUC meanI varI stddevI CVI maxI minI of a dataset inside the region -- as six moments per region.  This header is
// the single source of the logic.  It is compiled
//   * by hipcc for gfx950 inside csrc/wt_apply.hip (the product), and
//   * by g++ with -DWT_EMU inside tests/apply_emu.cpp, which runs the workgroups of every pass one after the other in any
//     order on the CPU.
// It is written in the manner of csrc/wt_cover.h and csrc/wt_region.h and uses their lane / sync macros, the single-workgroup
// scan of the former and the window of the latter: a region is to the dataset what a trim source run is to its mask.
//
// Input: a dataset D and regions R in the layout of wtamd_runs_map with the same number of segments; segment g of one pairs
// with segment g of the other.  D is sorted, start < finish and DISJOINT (start[i] >= finish[i-1]); R is sorted by start with
// start < finish and may overlap, nest or repeat: every region is evaluated on its own.  No start is negative.
//
// Region r = [rs, rf) of segment g:  lo = the first run of D's segment with finish > rs, hi = the first with start >= rf;
// the pieces are [max(s, rs), min(f, rf)) of the runs in [lo, hi) (only the first and the last can be clipped).  With L the
// piece lengths and v the values widened to f64:
//   m[0] = S L v    m[1] = span = S L    m[2] = T = S L (v - m[0]/m[1])^2    m[3] = min    m[4] = max      over the pieces whose
//   value is not NaN (min and max NaN when there is none: the meaning of wtamd_runs_moments), and
//   m[5] = covered = S L over ALL pieces, NaN-valued ones included.
// Fill-in mode (not WAP_STRICT): the (rf - rs) - covered uncovered base pairs enter with the default value, unless that is
// NaN, as ONE partial {sum U d, span U, T 0, min d, max d} merged after the data (a tie between the default and a data value
// that compare equal goes to the data); m[5] stays the data's covered length.
//
// Arithmetic (csrc/wt_moments_merge.h): every partial of one region is taken about one pivot K = the value of run lo (0 when
// that is NaN); a lane accumulates its runs in order about a pivot of its own and restates them about K; partials are merged
// pairwise in a fixed order.  A region's six doubles are a function of the region, its dataset segment, the default and the
// mode alone -- not of the other regions of the call, nor of the tile it falls in.
//
// Passes (no pass waits for another workgroup, no atomics on the results):
//   valid   one lane per interval, either side (wrg_valid_block)
//   bounds  a tile = WAP_TILE regions, WAP_PER_LANE consecutive ones per lane.  The tile meets a contiguous window of dataset
//           runs (wrg_window), staged in LDS when it holds at most WAP_WINDOW runs; every region does its two binary searches
//           and stores {lo, hi - lo}.  LANE REGIME: a region with at most WAP_SMALL runs under it is finished here by its own
//           lane, run by run in order, and no later pass touches it.  CHUNK REGIME: a larger region is cut into chunks of
//           WAP_CHUNK consecutive runs; the region stores the chunks before it inside the tile, the tile its chunk count.
//   scan    of the tiles' chunk counts (wcv_scan_block)
//   chunk   one wavefront per chunk (four per workgroup): two binary searches (tile, then region inside the tile) find the
//           chunk's region, consecutive lanes take consecutive runs, the 64 lanes merge pairwise through LDS, lane 0 writes
//           the partial.  Chunk count, not region count, sizes the pass.
//   final   one workgroup per chunk, which leaves at once unless the chunk is a region's FIRST; those merge the region's partials -- each lane a contiguous
//           share in chunk order, then the lanes pairwise -- then the fill-in partial, and write the six doubles.
//
// Scratch: 16 bytes per region + 64 bytes per chunk (+ 8 bytes per tile of 1024 regions); a chunk is 2048 runs of a region
// with more than 32, so at most n_runs / 2048 + 1 chunks per region.
#ifndef WT_APPLY_H_
#define WT_APPLY_H_

#include "wt_region.h"
#include "wt_moments_merge.h"

#define WAP_BLOCK WCV_BLOCK
#define WAP_PER_LANE 4
#define WAP_TILE (WAP_BLOCK * WAP_PER_LANE)     // regions per workgroup of the bounds pass
#define WAP_WINDOW WRG_WINDOW                   // dataset runs a tile stages in LDS (start + finish: 16 KiB)
#define WAP_SMALL 32                            // runs a lane finishes by itself
#define WAP_CHUNK 2048                          // runs one wavefront reduces: 32 per lane
#define WAP_WAVE 64
#define WAP_WAVES (WAP_BLOCK / WAP_WAVE)

#define WAP_STRICT 1u

enum { WAP_K_VALID_D = 0, WAP_K_VALID_R, WAP_K_BOUNDS, WAP_K_CHUNK, WAP_K_FINAL, WAP_K_COUNT_ };
enum { WAP_S_ERR = WRG_S_ERR, WAP_S_NCHUNK = WRG_S_NOUT, WAP_S_N = WRG_S_N };

struct WapRegion {          // 16 bytes
    long long lo;           // the first run under the region
    int nruns;              // hi - lo
    int cbase;              // chunks of the regions before it in its tile
};

struct WapAcc {
    WmAcc m;
    double cov;
};

struct WapPartial {         // 64 bytes
    double n, d, T, mn, mx;
    long long imn, imx;
    double cov;
};

struct WapLds {
    union {
        WrgLds rg;                  // bounds: the window and the lanes' chunk counts
        WapAcc acc[WAP_BLOCK];      // chunk, final: the lanes' partials
    };
    long long region;               // final: the region whose first chunk the workgroup stands for, -1: none
};

struct WapArgs {
    // dataset
    const int32_t *start, *finish;
    const void *value;
    int value_is_f64;
    const int64_t *seg_off;         // [n_seg + 1]
    long long n_seg, n;
    // regions
    const int32_t *r_start, *r_finish;
    const int64_t *r_seg_off;       // [n_seg + 1]
    long long n_r;
    double default_value;
    unsigned int flags;
    WapRegion *region;              // [n_r]
    long long *tile_cnt;            // [tiles] chunks of the tile, then chunks before the tile
    long long tiles, n_chunks;
    WapPartial *partial;            // [n_chunks]
    long long *scalars;
    double *out6;                   // [6 n_r]
};

WCV_DEV double wap_value(const WapArgs &a, long long k) {
    return a.value_is_f64 ? ((const double *) a.value)[k] : (double) ((const float *) a.value)[k];
}

// the pivot of a region whose first run is lo
WCV_DEV double wap_pivot(const WapArgs &a, long long lo) {
    const double v = wap_value(a, lo);
    return v == v ? v : 0.0;
}

// the regions as the source and the dataset as the mask of csrc/wt_region.h
WCV_DEV WrgArgs wap_as_region(const WapArgs &a) {
    WrgArgs r = {};
    r.op = WRG_TRIM;
    r.start = a.r_start; r.finish = a.r_finish; r.seg_off = a.r_seg_off; r.n_seg = a.n_seg; r.n = a.n_r;
    r.g_start = a.start; r.g_finish = a.finish; r.g_off = a.seg_off;
    r.scalars = a.scalars;
    return r;
}

// ---- valid ----
WCV_DEV void wap_valid_block(const WapArgs &a, bool regions, long long block, WapLds *lds) {
    WrgArgs r = wap_as_region(a);
    if (regions) { r.v_start = a.r_start; r.v_finish = a.r_finish; r.v_seg_off = a.r_seg_off; r.v_n = a.n_r; r.v_disjoint = 0; }
    else { r.v_start = a.start; r.v_finish = a.finish; r.v_seg_off = a.seg_off; r.v_n = a.n; r.v_disjoint = 1; }
    wrg_valid_block(r, block, &lds->rg);
    WCV_LANES(l) {                  // coordinates are not negative: no length or difference of two of them overflows an int32
        const long long i = block * WAP_BLOCK + l;
        if (i < r.v_n && r.v_start[i] < 0) wcv_add64(&a.scalars[WAP_S_ERR], 1);
    }
}

// piece of run k inside [rs, rf)
WCV_DEV void wap_add(const WapArgs &a, WmLane &lane, double &cov, long long k, int32_t s, int32_t f, int32_t rs, int32_t rf) {
    const int32_t ps = s > rs ? s : rs, pf = f < rf ? f : rf;
    cov += (double) (pf - ps);
    wm_add(lane, k, ps, pf, wap_value(a, k));
}

// the data's partial (about K) closed into the region's six doubles
WCV_DEV void wap_close(const WapArgs &a, WapAcc c, double K, int32_t rs, int32_t rf, double *out6) {
    const double d = a.default_value;
    if (!(a.flags & WAP_STRICT) && d == d) {
        const double U = (double) (rf - rs) - c.cov;
        if (U > 0) {
            WmAcc b;
            b.n = U; b.d = U * (d - K); b.T = 0.0; b.mn = b.mx = d; b.imn = b.imx = WM_NONE - 1;       // (after every run)
            wm_merge(c.m, b);
        }
    }
    out6[0] = c.m.n > 0 ? K * c.m.n + c.m.d : 0.0;
    out6[1] = c.m.n;
    out6[2] = c.m.T;
    out6[3] = c.m.imn != WM_NONE ? c.m.mn : __builtin_nan("");
    out6[4] = c.m.imx != WM_NONE ? c.m.mx : __builtin_nan("");
    out6[5] = c.cov;
}

WCV_DEV long long wap_chunks(long long nruns) { return nruns > WAP_SMALL ? (nruns + WAP_CHUNK - 1) / WAP_CHUNK : 0; }

// ---- bounds ----
WCV_DEV void wap_bounds_block(const WapArgs &a, long long tile, WapLds *lds) {
    const WrgArgs r = wap_as_region(a);
    wrg_window(r, tile, &lds->rg);
    WCV_LANES(l) {
        const WrgMask m = wrg_tile_mask(r, &lds->rg);
        long long cnt = 0;
        for (int q = 0; q < WAP_PER_LANE; q++) {
            const long long i = tile * WAP_TILE + (long long) l * WAP_PER_LANE + q;
            if (i >= a.n_r) break;
            long long lo, hi;
            wrg_span(r, m, i, wcv_seg_of(a.r_seg_off, a.n_seg, i), &lo, &hi);
            if (hi < lo) hi = lo;
            a.region[i].lo = lo;
            a.region[i].nruns = (int) (hi - lo);
            const long long c = wap_chunks(hi - lo);
            cnt += c;
            if (c) continue;
            // lane regime: run by run, in order
            const int32_t rs = a.r_start[i], rf = a.r_finish[i];
            WmLane lane = wm_lane_zero();
            WapAcc acc;
            acc.cov = 0.0;
            const double K = hi > lo ? wap_pivot(a, lo) : 0.0;
            for (long long k = lo; k < hi; k++) wap_add(a, lane, acc.cov, k, m.s(k), m.f(k), rs, rf);
            acc.m = wm_lane_acc(lane, K);
            wap_close(a, acc, K, rs, rf, a.out6 + 6 * i);
        }
        lds->rg.off[l] = cnt;
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (l == 0) {
            long long run = 0;
            for (int k = 0; k < WAP_BLOCK; k++) { const long long c = lds->rg.off[k]; lds->rg.off[k] = run; run += c; }
            a.tile_cnt[tile] = run;
        }
    }
    WCV_SYNC();
    WCV_LANES(l) {
        long long run = lds->rg.off[l];
        for (int q = 0; q < WAP_PER_LANE; q++) {
            const long long i = tile * WAP_TILE + (long long) l * WAP_PER_LANE + q;
            if (i >= a.n_r) break;
            a.region[i].cbase = (int) run;
            run += wap_chunks(a.region[i].nruns);
        }
    }
}

// chunk q of the call (tile_cnt scanned) -> its region and the chunk inside it.  A tile or a region without chunks has the base
// of the one after it, so "the last one whose base is <= q" is the one that holds q.
WCV_DEV void wap_locate(const WapArgs &a, long long q, long long *region, long long *chunk) {
    long long b0 = 0, b1 = a.tiles;                 // tile_cnt[b0] <= q < tile_cnt[b1]
    while (b1 - b0 > 1) { const long long mid = (b0 + b1) >> 1; if (a.tile_cnt[mid] <= q) b0 = mid; else b1 = mid; }
    const long long ql = q - a.tile_cnt[b0];
    long long r0 = b0 * WAP_TILE, r1 = r0 + WAP_TILE < a.n_r ? r0 + WAP_TILE : a.n_r;
    while (r1 - r0 > 1) { const long long mid = (r0 + r1) >> 1; if ((long long) a.region[mid].cbase <= ql) r0 = mid; else r1 = mid; }
    *region = r0;
    *chunk = ql - a.region[r0].cbase;
}

// lanes [base, base + width) of lds->acc merged pairwise, lower lane first; acc[base] ends up with all of them
WCV_DEV void wap_tree(WapLds *lds, int width) {
    for (int s = 1; s < width; s <<= 1) {
        WCV_SYNC();
        WCV_LANES(l) {
            if ((l & (2 * s - 1)) == 0) {
                wm_merge(lds->acc[l].m, lds->acc[l + s].m);
                lds->acc[l].cov += lds->acc[l + s].cov;
            }
        }
    }
    WCV_SYNC();
}

// ---- chunk: wave w of workgroup b reduces chunk 4 b + w ----
WCV_DEV void wap_chunk_block(const WapArgs &a, long long block, WapLds *lds) {
    WCV_LANES(l) {
        const int w = l / WAP_WAVE, j = l % WAP_WAVE;
        const long long q = block * WAP_WAVES + w;
        WmLane lane = wm_lane_zero();
        WapAcc acc;
        acc.cov = 0.0;
        double K = 0.0;
        if (q < a.n_chunks) {
            long long i, c;
            wap_locate(a, q, &i, &c);
            const WapRegion rg = a.region[i];
            const int32_t rs = a.r_start[i], rf = a.r_finish[i];
            const long long k0 = rg.lo + c * WAP_CHUNK, hi = rg.lo + rg.nruns, k1 = k0 + WAP_CHUNK < hi ? k0 + WAP_CHUNK : hi;
            K = wap_pivot(a, rg.lo);
            for (long long k = k0 + j; k < k1; k += WAP_WAVE) wap_add(a, lane, acc.cov, k, a.start[k], a.finish[k], rs, rf);
        }
        acc.m = wm_lane_acc(lane, K);
        lds->acc[l] = acc;
    }
    wap_tree(lds, WAP_WAVE);
    WCV_LANES(l) {
        const long long q = block * WAP_WAVES + l / WAP_WAVE;
        if (l % WAP_WAVE == 0 && q < a.n_chunks) {
            const WapAcc c = lds->acc[l];
            WapPartial p;
            p.n = c.m.n; p.d = c.m.d; p.T = c.m.T; p.mn = c.m.mn; p.mx = c.m.mx; p.imn = c.m.imn; p.imx = c.m.imx; p.cov = c.cov;
            a.partial[q] = p;
        }
    }
}

// ---- final: workgroup q, when chunk q is the first of its region, merges the region's partials ----
WCV_DEV void wap_final_block(const WapArgs &a, long long block, WapLds *lds) {
    WCV_LANES(l) {
        if (l == 0) {
            long long i, c;
            wap_locate(a, block, &i, &c);
            lds->region = c == 0 ? i : -1;
        }
    }
    WCV_SYNC();
    if (lds->region < 0) return;            // (the whole workgroup: a later chunk of a region has nothing to do)
    WCV_LANES(l) {
        WapAcc acc;
        acc.m.n = acc.m.d = acc.m.T = acc.m.mn = acc.m.mx = 0.0; acc.m.imn = acc.m.imx = WM_NONE; acc.cov = 0.0;
        const long long i = lds->region;
        if (i >= 0) {
            const long long parts = wap_chunks(a.region[i].nruns), per = (parts + WAP_BLOCK - 1) / WAP_BLOCK;
            for (long long c = (long long) l * per; c < ((long long) l + 1) * per && c < parts; c++) {
                const WapPartial p = a.partial[block + c];
                WmAcc b = {p.n, p.d, p.T, p.mn, p.mx, p.imn, p.imx};
                wm_merge(acc.m, b);
                acc.cov += p.cov;
            }
        }
        lds->acc[l] = acc;
    }
    wap_tree(lds, WAP_BLOCK);
    WCV_LANES(l) {
        const long long i = lds->region;
        if (l == 0 && i >= 0) wap_close(a, lds->acc[0], wap_pivot(a, a.region[i].lo), a.r_start[i], a.r_finish[i], a.out6 + 6 * i);
    }
}

WCV_DEV void wap_run_block(int kernel, const WapArgs &a, long long block, WapLds *lds) {
    switch (kernel) {
    case WAP_K_VALID_D: wap_valid_block(a, false, block, lds); break;
    case WAP_K_VALID_R: wap_valid_block(a, true, block, lds); break;
    case WAP_K_BOUNDS: wap_bounds_block(a, block, lds); break;
    case WAP_K_CHUNK: wap_chunk_block(a, block, lds); break;
    case WAP_K_FINAL: wap_final_block(a, block, lds); break;
    default: break;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The door, written once over a Launcher: the one of wt_cover.h (alloc, release, zero, to_host, to_device, run over WcvArgs)
// with    bool run_apply(int kernel, long long blocks, const WapArgs &a)     and     bool sync()
// Return value: 0 fine, 1 bad argument, 2 launcher failure (the WTAMD_* codes).  Nothing is written to moments6 unless the
// value is 0.
// ---------------------------------------------------------------------------------------------------------------------
#ifndef WCV_NO_HOST

// The opening of this door and of the one of wt_profile.h.  wap_open_check: the host's look at the segment offsets; a.n_seg,
// a.start ... a.r_finish are set, a.n and a.n_r are set here; bad: what the door's own arguments (flags, width) already
// refuse; out, out_always: the output is needed where there are regions, or always.  wap_open: d_seg / d_rseg on the device,
// the scalars zeroed, the two validation passes -- valid(regions, blocks) launches the door's own instantiation -- and their
// verdict.
static int wap_open_check(WapArgs &a, const int64_t *seg_off, const int64_t *r_seg_off, bool bad, const void *out, bool out_always, const char **why) {
    const long long n_seg = a.n_seg;
    *why = "bad argument";
    if (n_seg < 0 || !seg_off || !r_seg_off || n_seg >= (1ll << 31) || bad) return 1;
    if (n_seg && (seg_off[0] != 0 || r_seg_off[0] != 0)) return 1;
    for (long long g = 0; g < n_seg; g++)
        if (seg_off[g + 1] < seg_off[g] || r_seg_off[g + 1] < r_seg_off[g]) { *why = "segment offsets decrease"; return 1; }
    a.n = n_seg ? (long long) seg_off[n_seg] : 0; a.n_r = n_seg ? (long long) r_seg_off[n_seg] : 0;
    if ((a.n > 0 && (!a.start || !a.finish || !a.value)) || (a.n_r > 0 && (!a.r_start || !a.r_finish)) || ((a.n_r > 0 || out_always) && !out)) return 1;
    if (a.n >= (1ll << 31)) { *why = "more than 2^31 - 1 dataset runs"; return 1; }
    *why = "";
    return 0;
}

template <class L, class Valid>
static int wap_open(L &l, WcvScope<L> &sc, WapArgs &a, const int64_t *seg_off, const int64_t *r_seg_off, Valid valid, const char **why) {
    const size_t n_off = (size_t) a.n_seg + 1;
    int64_t *d_seg = nullptr, *d_rseg = nullptr;
    if (!sc.get(&d_seg, n_off) || !sc.get(&d_rseg, n_off) || !sc.get(&a.scalars, (size_t) WAP_S_N)) { *why = "device memory"; return 2; }
    if (!l.to_device(d_seg, seg_off, sizeof(int64_t) * n_off) || !l.to_device(d_rseg, r_seg_off, sizeof(int64_t) * n_off) ||
        !l.zero(a.scalars, sizeof(long long) * WAP_S_N))
        { *why = "copy"; return 2; }
    a.seg_off = d_seg; a.r_seg_off = d_rseg;
    long long h_sc[WAP_S_N];
    if (!valid(false, wcv_blocks(a.n, WAP_BLOCK)) || !valid(true, wcv_blocks(a.n_r, WAP_BLOCK)) || !l.to_host(h_sc, a.scalars, sizeof h_sc))
        { *why = "validation pass"; return 2; }
    if (h_sc[WAP_S_ERR]) {
        *why = "a segment is not sorted by start, holds an interval with start < 0 or start >= finish, or is a dataset that overlaps itself";
        return 1;
    }
    return 0;
}

template <class L>
static int wap_apply(L &l, long long n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish, const void *value,
                     int value_is_f64, const int64_t *r_seg_off, const int32_t *r_start, const int32_t *r_finish, double default_value,
                     unsigned int flags, double *moments6, const char **why) {
    WapArgs a = {};
    a.n_seg = n_seg;
    a.start = start; a.finish = finish; a.value = value; a.value_is_f64 = value_is_f64;
    a.r_start = r_start; a.r_finish = r_finish;
    a.default_value = default_value; a.flags = flags; a.out6 = moments6;
    if (const int rc = wap_open_check(a, seg_off, r_seg_off, (flags & ~WAP_STRICT) != 0, moments6, false, why)) return rc;
    const long long n_r = a.n_r;
    WcvScope<L> sc(l);
    if (const int rc = wap_open(l, sc, a, seg_off, r_seg_off,
                                [&](bool regions, long long blocks) { return l.run_apply(regions ? WAP_K_VALID_R : WAP_K_VALID_D, blocks, a); }, why))
        return rc;
    long long h_sc[WAP_S_N];
    if (n_r == 0) return 0;
    a.tiles = wcv_blocks(n_r, WAP_TILE);
    if (!sc.get(&a.region, (size_t) n_r) || !sc.get(&a.tile_cnt, (size_t) a.tiles)) { *why = "device memory"; return 2; }
    WcvArgs s = {};
    s.scan = a.tile_cnt; s.scan_n = a.tiles; s.scan_init = nullptr; s.scan_total = &a.scalars[WAP_S_NCHUNK];
    if (!l.run_apply(WAP_K_BOUNDS, a.tiles, a) || !l.run(WCV_K_SCAN_SUM, 1, s) || !l.to_host(h_sc, a.scalars, sizeof h_sc))
        { *why = "bounds pass"; return 2; }
    a.n_chunks = h_sc[WAP_S_NCHUNK];
    if (a.n_chunks > 0) {
        if (!sc.get(&a.partial, (size_t) a.n_chunks)) { *why = "device memory"; return 2; }
        if (!l.run_apply(WAP_K_CHUNK, wcv_blocks(a.n_chunks, WAP_WAVES), a) || !l.run_apply(WAP_K_FINAL, a.n_chunks, a)) { *why = "chunk passes"; return 2; }
    }
    if (!l.sync()) { *why = "synchronisation"; return 2; }
    return 0;
}

#endif  // WCV_NO_HOST

// The same rules on the host, without a device (a translation unit compiled with -DWT_EMU: the arithmetic above is then plain
// C++): one segment pair, one sweep (the regions' lo only moves forward; a region restarts at its own lo).  Every region's
// runs are taken in order about the region's pivot, as the lane regime takes them.
#ifdef WT_EMU
static int wap_apply_host(long long n, const int32_t *start, const int32_t *finish, const double *value, long long n_r,
                          const int32_t *r_start, const int32_t *r_finish, double default_value, unsigned int flags, double *moments6) {
    if (n < 0 || n_r < 0 || (flags & ~WAP_STRICT) || (n > 0 && (!start || !finish || !value)) || (n_r > 0 && (!r_start || !r_finish || !moments6)))
        return 1;
    for (long long i = 0; i < n; i++) if (start[i] < 0 || start[i] >= finish[i] || (i > 0 && finish[i - 1] > start[i])) return 1;
    for (long long i = 0; i < n_r; i++) if (r_start[i] < 0 || r_start[i] >= r_finish[i] || (i > 0 && r_start[i - 1] > r_start[i])) return 1;
    WapArgs a = {};
    a.value = value; a.value_is_f64 = 1; a.default_value = default_value; a.flags = flags;
    long long lo = 0;
    for (long long i = 0; i < n_r; i++) {
        const int32_t rs = r_start[i], rf = r_finish[i];
        while (lo < n && finish[lo] <= rs) lo++;
        WmLane lane = wm_lane_zero();
        WapAcc acc;
        acc.cov = 0.0;
        const double K = lo < n && start[lo] < rf ? wap_pivot(a, lo) : 0.0;
        for (long long k = lo; k < n && start[k] < rf; k++) wap_add(a, lane, acc.cov, k, start[k], finish[k], rs, rf);
        acc.m = wm_lane_acc(lane, K);
        wap_close(a, acc, K, rs, rf, moments6 + 6 * i);
    }
    return 0;
}
#endif  // WT_EMU

#endif  // WT_APPLY_H_
