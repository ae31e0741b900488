// wt_region.h -- the reference's region operators over whole run lists (device + -DWT_EMU): OverlapWiggleIterator,
// TrimWiggleIterator, NoverlapWiggleIterator and NearestWiggleIterator (src/unaryOps.c:437-639; the parser's `overlaps`,
// `trim`, `noverlaps`, `nearest`, commandParser.c:813-819).  This header is the single source of the logic.  It is compiled
//   * by hipcc for gfx950 inside csrc/wt_region.hip (the product), and
//   * by g++ with -DWT_EMU inside tests/region_emu.cpp, which runs the workgroups of every pass one after the other in any
//     order on the CPU.
// It is written in the manner of csrc/wt_cover.h and uses its lane / sync macros, its single-workgroup scan and its union.
//
// Input: a source and a mask in the layout of wtamd_runs_map, with the same number of segments; segment g of one pairs with
// segment g of the other.  Inside a segment both are sorted by start and start < finish; either may overlap itself, except
// the source of a trim.
//
// Per segment, with S the source, M the raw mask and G = union(M) as wcv_union defines it (touching intervals stay apart;
// G.start and G.finish both increase strictly):
//   lo(i) = the first group with G.finish > S.start[i]            hi(i) = the first group with G.start >= S.finish[i]
//   overlaps    run i iff hi(i) > lo(i), carried unchanged
//   noverlaps   run i iff hi(i) <= lo(i)
//   trim        for g in [lo(i), hi(i)): [max(S.start, G.start[g]), min(S.finish, G.finish[g])) with the value of run i
//   nearest     k = #(M.start <= S.start[i]) over the RAW mask; the value is the smaller of S.start - M.finish[k-1] + 1 (if
//               k > 0) and M.start[k] - S.finish + 1 (if k < m) in int32 arithmetic, 0 where that is negative, NaN with no
//               candidate; start and finish carried.  (The reference's quirks stay: the + 1; "previous" is the mask that
//               STARTED last, whichever ends last; an enclosing earlier mask is not seen.)
// Values are carried bit for bit, widened to f64.
//
// Passes (no pass waits for another workgroup):
//   valid   one lane per interval: sorted by start, start < finish, for a trim source start[i] >= finish[i-1]
//   union   of the mask (wcv_union), not for nearest
//   count   a tile = WRG_TILE source runs, WRG_PER_LANE consecutive ones per lane.  Lane 0 finds the window of mask
//           groups the tile can meet -- from lo of its first run to hi of the largest finish among the runs of its last
//           segment (starts are sorted, finishes need not be) --, the workgroup stages it in LDS when it holds at most
//           WRG_WINDOW groups, and every run does its two binary searches inside the window, in LDS or in global memory.
//   scan    of the tile counts (wcv_scan_block)
//   emit    the same searches again, an exclusive scan of the lanes' counts, every lane writes its runs' outputs in order
//           (a trim run that meets many groups writes all of them); the first run of a segment writes the segment's offset.
#ifndef WT_REGION_H_
#define WT_REGION_H_

#include "wt_cover.h"

#define WRG_BLOCK WCV_BLOCK
#define WRG_PER_LANE 4
#define WRG_TILE (WRG_BLOCK * WRG_PER_LANE)      // T: source runs per workgroup
#define WRG_WINDOW 2048                          // W: mask groups a workgroup stages in LDS (16 KiB)

enum { WRG_OVERLAPS = 0, WRG_NOVERLAPS = 1, WRG_TRIM = 2, WRG_NEAREST = 3, WRG_OP_COUNT_ };
enum { WRG_K_VALID = 0, WRG_K_COUNT, WRG_K_EMIT, WRG_K_COUNT_ };
enum { WRG_S_ERR = 0 /* != 0: a refused interval */, WRG_S_NOUT = 1 /* runs the call emits */, WRG_S_N = 4 };

struct WrgLds {
    int32_t gs[WRG_WINDOW], gf[WRG_WINDOW];     // the staged window of the mask
    long long off[WRG_BLOCK];
    unsigned int cnt[WRG_BLOCK];
    long long wa, wb;                           // the window: mask groups [wa, wb)
    long long last_seg;
    int maxfin;
    int staged;
};

struct WrgArgs {
    int op;
    // valid: the list it checks
    const int32_t *v_start, *v_finish;
    const int64_t *v_seg_off;
    long long v_n;
    int v_disjoint;                 // also refuse start[i] < finish[i-1]
    // source
    const int32_t *start, *finish;
    const void *value;
    int value_is_f64;
    const int64_t *seg_off;         // [n_seg + 1]
    long long n_seg, n;
    // mask: the union's groups, or the raw mask for nearest
    const int32_t *g_start, *g_finish;
    const int64_t *g_off;           // [n_seg + 1]
    long long *tile_cnt;            // [tiles] outputs of the tile, then outputs before the tile
    long long *scalars;
    // output
    int32_t *o_start, *o_finish;
    double *o_value;
    long long capacity;
    int64_t *o_seg;                 // [n_seg + 1] device copy of the output offsets (non-empty segments)
};

// ---- valid ----
WCV_DEV void wrg_valid_block(const WrgArgs &a, long long block, WrgLds *) {
    WCV_LANES(l) {
        const long long i = block * WRG_BLOCK + l;
        if (i >= a.v_n) continue;
        const long long g = wcv_seg_of(a.v_seg_off, a.n_seg, i);
        const int32_t s = a.v_start[i], f = a.v_finish[i];
        bool bad = s >= f;
        if (i > (long long) a.v_seg_off[g] && (a.v_start[i - 1] > s || (a.v_disjoint && a.v_finish[i - 1] > s))) bad = true;
        if (bad) wcv_add64(&a.scalars[WRG_S_ERR], 1);
    }
}

// The mask as a tile sees it: groups [wa, wb) from LDS when staged, everything else from global memory.
struct WrgMask {
    const int32_t *gs, *gf;         // global
    const int32_t *ls, *lf;         // the staged window
    long long wa, wb;
    bool staged;
    WCV_DEV int32_t s(long long k) const { return staged && k >= wa && k < wb ? ls[k - wa] : gs[k]; }
    WCV_DEV int32_t f(long long k) const { return staged && k >= wa && k < wb ? lf[k - wa] : gf[k]; }
    // the first k in [b0, b1) with finish > x / start >= x / start > x; b1 when there is none
    WCV_DEV long long first_finish_gt(long long b0, long long b1, int32_t x) const {
        while (b0 < b1) { const long long mid = (b0 + b1) >> 1; if (f(mid) > x) b1 = mid; else b0 = mid + 1; }
        return b0;
    }
    WCV_DEV long long first_start_ge(long long b0, long long b1, int32_t x) const {
        while (b0 < b1) { const long long mid = (b0 + b1) >> 1; if (s(mid) >= x) b1 = mid; else b0 = mid + 1; }
        return b0;
    }
    WCV_DEV long long first_start_gt(long long b0, long long b1, int32_t x) const {
        while (b0 < b1) { const long long mid = (b0 + b1) >> 1; if (s(mid) > x) b1 = mid; else b0 = mid + 1; }
        return b0;
    }
};

WCV_DEV WrgMask wrg_global_mask(const WrgArgs &a) {
    WrgMask m;
    m.gs = a.g_start; m.gf = a.g_finish; m.ls = nullptr; m.lf = nullptr; m.wa = 0; m.wb = 0; m.staged = false;
    return m;
}

// The window of the tile and its copy in LDS.  Every search of a run of the tile has its answer inside [wa, wb]:
// starts are sorted inside a segment, so no run begins its groups before the tile's first run does, and no run of the last
// segment ends them after the largest finish does; the segments between lie between.
WCV_DEV void wrg_window(const WrgArgs &a, long long tile, WrgLds *lds) {
    const long long i0 = tile * WRG_TILE, i1 = i0 + WRG_TILE < a.n ? i0 + WRG_TILE : a.n;
    WCV_LANES(l) {
        if (l == 0) { lds->maxfin = INT32_MIN; lds->last_seg = wcv_seg_of(a.seg_off, a.n_seg, i1 - 1); }
    }
    WCV_SYNC();
    if (a.op != WRG_NEAREST) {
        WCV_LANES(l) {
            const long long first = (long long) a.seg_off[lds->last_seg];
            int32_t m = INT32_MIN;
            for (int k = 0; k < WRG_PER_LANE; k++) {
                const long long i = i0 + (long long) l * WRG_PER_LANE + k;
                if (i < i1 && i >= first && a.finish[i] > m) m = a.finish[i];
            }
            if (m != INT32_MIN) wcv_max32(&lds->maxfin, m);
        }
        WCV_SYNC();
    }
    WCV_LANES(l) {
        if (l == 0) {
            const WrgMask g = wrg_global_mask(a);
            const long long g0 = wcv_seg_of(a.seg_off, a.n_seg, i0), g1 = lds->last_seg;
            long long wa, wb;
            if (a.op == WRG_NEAREST) {
                const long long k0 = g.first_start_gt((long long) a.g_off[g0], (long long) a.g_off[g0 + 1], a.start[i0]);
                const long long k1 = g.first_start_gt((long long) a.g_off[g1], (long long) a.g_off[g1 + 1], a.start[i1 - 1]);
                wa = k0 > (long long) a.g_off[g0] ? k0 - 1 : k0;                    // (the previous mask is read too)
                wb = k1 < (long long) a.g_off[g1 + 1] ? k1 + 1 : k1;                // (and the next)
            } else {
                wa = g.first_finish_gt((long long) a.g_off[g0], (long long) a.g_off[g0 + 1], a.start[i0]);
                wb = g.first_start_ge((long long) a.g_off[g1], (long long) a.g_off[g1 + 1], lds->maxfin);
            }
            if (wb < wa) wb = wa;
            lds->wa = wa; lds->wb = wb;
            lds->staged = wb - wa <= WRG_WINDOW;
        }
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (lds->staged)
            for (long long k = l; k < lds->wb - lds->wa; k += WRG_BLOCK) {
                lds->gs[k] = a.g_start[lds->wa + k];
                lds->gf[k] = a.g_finish[lds->wa + k];
            }
    }
    WCV_SYNC();
}

WCV_DEV WrgMask wrg_tile_mask(const WrgArgs &a, const WrgLds *lds) {
    WrgMask m;
    m.gs = a.g_start; m.gf = a.g_finish; m.ls = lds->gs; m.lf = lds->gf; m.wa = lds->wa; m.wb = lds->wb; m.staged = lds->staged != 0;
    return m;
}

// run i of segment g: for overlaps / noverlaps / trim the groups [*lo, *hi) it meets, for nearest *lo = k.  Returns the
// number of runs it puts out.
WCV_DEV long long wrg_span(const WrgArgs &a, const WrgMask &m, long long i, long long g, long long *lo, long long *hi) {
    long long b0 = (long long) a.g_off[g], b1 = (long long) a.g_off[g + 1];
    if (b0 < m.wa) b0 = m.wa;
    if (b1 > m.wb) b1 = m.wb;
    if (b1 < b0) b1 = b0;
    if (a.op == WRG_NEAREST) {
        *lo = *hi = m.first_start_gt(b0, b1, a.start[i]);
        return 1;
    }
    *lo = m.first_finish_gt(b0, b1, a.start[i]);
    *hi = m.first_start_ge(*lo, b1, a.finish[i]);
    if (a.op == WRG_TRIM) return *hi - *lo;
    return (a.op == WRG_OVERLAPS) == (*hi > *lo) ? 1 : 0;
}

// ---- count ----
WCV_DEV void wrg_count_block(const WrgArgs &a, long long tile, WrgLds *lds) {
    wrg_window(a, tile, lds);
    WCV_LANES(l) {
        const WrgMask m = wrg_tile_mask(a, lds);
        long long cnt = 0;
        for (int k = 0; k < WRG_PER_LANE; k++) {
            const long long i = tile * WRG_TILE + (long long) l * WRG_PER_LANE + k;
            if (i >= a.n) break;
            long long lo, hi;
            cnt += wrg_span(a, m, i, wcv_seg_of(a.seg_off, a.n_seg, i), &lo, &hi);
        }
        lds->off[l] = cnt;
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (l == 0) {
            long long run = 0;
            for (int k = 0; k < WRG_BLOCK; k++) run += lds->off[k];
            a.tile_cnt[tile] = run;
        }
    }
}

// bit for bit: a NaN keeps its payload, -0.0 its sign (f32 widens exactly)
WCV_DEV unsigned long long wrg_value_bits(const WrgArgs &a, long long i) {
    if (a.value_is_f64) return ((const unsigned long long *) a.value)[i];
    union { double d; unsigned long long u; } w;
    w.d = (double) ((const float *) a.value)[i];
    return w.u;
}

// nearest: the distance of run i to the mask that started last before or at its start, or to the next one
WCV_DEV unsigned long long wrg_nearest_bits(const WrgArgs &a, const WrgMask &m, long long i, long long g, long long k) {
    bool set = false;
    int32_t best = 0;
    if (k > (long long) a.g_off[g]) {
        best = (int32_t) ((uint32_t) a.start[i] - (uint32_t) m.f(k - 1) + 1u);
        set = true;
    }
    if (k < (long long) a.g_off[g + 1]) {
        const int32_t c = (int32_t) ((uint32_t) m.s(k) - (uint32_t) a.finish[i] + 1u);
        if (!set || best > c) best = c;
        set = true;
    }
    if (!set) return 0x7ff8000000000000ull;
    union { double d; unsigned long long u; } w;
    w.d = best < 0 ? 0.0 : (double) best;
    return w.u;
}

// ---- emit (tile_cnt scanned: outputs before the tile) ----
WCV_DEV void wrg_emit_block(const WrgArgs &a, long long tile, WrgLds *lds) {
    wrg_window(a, tile, lds);
    WCV_LANES(l) {
        const WrgMask m = wrg_tile_mask(a, lds);
        long long cnt = 0;
        for (int k = 0; k < WRG_PER_LANE; k++) {
            const long long i = tile * WRG_TILE + (long long) l * WRG_PER_LANE + k;
            if (i >= a.n) break;
            long long lo, hi;
            cnt += wrg_span(a, m, i, wcv_seg_of(a.seg_off, a.n_seg, i), &lo, &hi);
        }
        lds->off[l] = cnt;
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (l == 0) {
            long long run = a.tile_cnt[tile];
            for (int k = 0; k < WRG_BLOCK; k++) { const long long c = lds->off[k]; lds->off[k] = run; run += c; }
        }
    }
    WCV_SYNC();
    WCV_LANES(l) {
        const WrgMask m = wrg_tile_mask(a, lds);
        long long o = lds->off[l];
        for (int k = 0; k < WRG_PER_LANE; k++) {
            const long long i = tile * WRG_TILE + (long long) l * WRG_PER_LANE + k;
            if (i >= a.n) break;
            const long long g = wcv_seg_of(a.seg_off, a.n_seg, i);
            if (i == (long long) a.seg_off[g]) a.o_seg[g] = (int64_t) o;
            long long lo, hi;
            const long long c = wrg_span(a, m, i, g, &lo, &hi);
            if (c == 0) continue;
            const int32_t s = a.start[i], f = a.finish[i];
            if (a.op == WRG_TRIM) {
                const unsigned long long bits = wrg_value_bits(a, i);
                for (long long q = lo; q < hi; q++, o++) {
                    if (o >= a.capacity) continue;
                    const int32_t ms = m.s(q), mf = m.f(q);
                    a.o_start[o] = s > ms ? s : ms;
                    a.o_finish[o] = f < mf ? f : mf;
                    ((unsigned long long *) a.o_value)[o] = bits;
                }
                continue;
            }
            if (o < a.capacity) {
                a.o_start[o] = s;
                a.o_finish[o] = f;
                ((unsigned long long *) a.o_value)[o] = a.op == WRG_NEAREST ? wrg_nearest_bits(a, m, i, g, lo) : wrg_value_bits(a, i);
            }
            o++;
        }
    }
}

WCV_DEV void wrg_run_block(int kernel, const WrgArgs &a, long long block, WrgLds *lds) {
    switch (kernel) {
    case WRG_K_VALID: wrg_valid_block(a, block, lds); break;
    case WRG_K_COUNT: wrg_count_block(a, block, lds); break;
    case WRG_K_EMIT: wrg_emit_block(a, block, lds); break;
    default: break;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The door, written once over a Launcher: the one of wt_cover.h (alloc, release, zero, to_host, to_device, run over WcvArgs)
// with    bool run_region(int kernel, long long blocks, const WrgArgs &a)
// Return value: 0 fine, 1 bad argument, 2 launcher failure, 3 capacity (the WTAMD_* codes).  Nothing is written to the
// output arrays unless the value is 0.
// ---------------------------------------------------------------------------------------------------------------------
#ifndef WCV_NO_HOST

template <class L>
static int wrg_region(L &l, int op, long long n_seg, const int64_t *seg_off, const int32_t *start, const int32_t *finish, const void *value,
                      int value_is_f64, const int64_t *m_seg_off, const int32_t *m_start, const int32_t *m_finish, long long capacity,
                      int32_t *o_start, int32_t *o_finish, double *o_value, int64_t *o_seg_off, int64_t *n_out, const char **why) {
    *why = "";
    if (op < 0 || op >= WRG_OP_COUNT_) { *why = "unknown operator"; return 1; }
    if (n_seg < 0 || !seg_off || !m_seg_off || !o_seg_off || !n_out || capacity < 0 || n_seg >= (1ll << 31)) { *why = "bad argument"; return 1; }
    if (n_seg && (seg_off[0] != 0 || m_seg_off[0] != 0)) { *why = "bad argument"; return 1; }
    for (long long g = 0; g < n_seg; g++)
        if (seg_off[g + 1] < seg_off[g] || m_seg_off[g + 1] < m_seg_off[g]) { *why = "segment offsets decrease"; return 1; }
    const long long n = n_seg ? (long long) seg_off[n_seg] : 0, m = n_seg ? (long long) m_seg_off[n_seg] : 0;
    if ((n > 0 && (!start || !finish || !value)) || (m > 0 && (!m_start || !m_finish))) { *why = "bad argument"; return 1; }
    *n_out = 0;
    static const char *const refused = "a segment is not sorted by start, holds an interval with start >= finish, or is a trim source that overlaps itself";
    WcvScope<L> sc(l);
    WrgArgs a = {};
    a.op = op; a.n_seg = n_seg; a.n = n;
    a.start = start; a.finish = finish; a.value = value; a.value_is_f64 = value_is_f64;
    a.o_start = o_start; a.o_finish = o_finish; a.o_value = o_value; a.capacity = capacity;
    int64_t *d_seg = nullptr, *d_goff = nullptr;
    if (!sc.get(&d_seg, (size_t) n_seg + 1) || !sc.get(&d_goff, (size_t) n_seg + 1) || !sc.get(&a.scalars, (size_t) WRG_S_N) ||
        !sc.get(&a.o_seg, (size_t) n_seg + 1))
        { *why = "device memory"; return 2; }
    if (!l.to_device(d_seg, seg_off, sizeof(int64_t) * ((size_t) n_seg + 1)) || !l.to_device(d_goff, m_seg_off, sizeof(int64_t) * ((size_t) n_seg + 1)) ||
        !l.zero(a.scalars, sizeof(long long) * WRG_S_N) || !l.zero(a.o_seg, sizeof(int64_t) * ((size_t) n_seg + 1)))
        { *why = "copy"; return 2; }
    a.seg_off = d_seg;
    // validation: the source, and the mask where the union will not see it
    bool ok = true;
    a.v_start = start; a.v_finish = finish; a.v_seg_off = d_seg; a.v_n = n; a.v_disjoint = op == WRG_TRIM;
    ok = ok && l.run_region(WRG_K_VALID, wcv_blocks(n, WRG_BLOCK), a);
    if (op == WRG_NEAREST || n == 0) {
        a.v_start = m_start; a.v_finish = m_finish; a.v_seg_off = d_goff; a.v_n = m; a.v_disjoint = 0;
        ok = ok && l.run_region(WRG_K_VALID, wcv_blocks(m, WRG_BLOCK), a);
    }
    long long h_sc[WRG_S_N];
    if (!ok || !l.to_host(h_sc, a.scalars, sizeof h_sc)) { *why = "validation pass"; return 2; }
    if (h_sc[WRG_S_ERR]) { *why = refused; return 1; }
    if (capacity > 0 && (!o_start || !o_finish || !o_value)) { *why = "bad argument"; return 1; }
    // the mask the searches see
    a.g_start = m_start; a.g_finish = m_finish; a.g_off = d_goff;
    if (op != WRG_NEAREST && m > 0 && n > 0) {
        int32_t *u_start = nullptr, *u_finish = nullptr;
        if (!sc.get(&u_start, (size_t) m) || !sc.get(&u_finish, (size_t) m)) { *why = "device memory"; return 2; }
        std::vector<int64_t> h_goff((size_t) n_seg + 1);
        int64_t n_groups = 0;
        const char *uwhy = "";
        const int rc = wcv_union(l, n_seg, m_seg_off, m_start, m_finish, nullptr, 0, m, u_start, u_finish, nullptr, h_goff.data(), &n_groups, &uwhy);
        if (rc == 1) { *why = refused; return 1; }
        if (rc != 0) { *why = "union of the mask"; return 2; }
        if (!l.to_device(d_goff, h_goff.data(), sizeof(int64_t) * h_goff.size())) { *why = "copy"; return 2; }
        a.g_start = u_start; a.g_finish = u_finish;
    }
    if (n == 0) { for (long long g = 0; g <= n_seg; g++) o_seg_off[g] = 0; return 0; }
    const long long tiles = wcv_blocks(n, WRG_TILE);
    if (!sc.get(&a.tile_cnt, (size_t) tiles)) { *why = "device memory"; return 2; }
    WcvArgs s = {};
    s.scan = a.tile_cnt; s.scan_n = tiles; s.scan_init = nullptr; s.scan_total = &a.scalars[WRG_S_NOUT];
    if (!l.run_region(WRG_K_COUNT, tiles, a) || !l.run(WCV_K_SCAN_SUM, 1, s) || !l.to_host(h_sc, a.scalars, sizeof h_sc))
        { *why = "count passes"; return 2; }
    const long long out = h_sc[WRG_S_NOUT];
    *n_out = out;
    if (out > capacity) return 3;
    std::vector<int64_t> h_oseg((size_t) n_seg + 1);
    if (!l.run_region(WRG_K_EMIT, tiles, a) || !l.to_host(h_oseg.data(), a.o_seg, sizeof(int64_t) * h_oseg.size())) { *why = "emit pass"; return 2; }
    o_seg_off[n_seg] = out;
    for (long long q = n_seg - 1; q >= 0; q--) o_seg_off[q] = seg_off[q + 1] == seg_off[q] ? o_seg_off[q + 1] : h_oseg[(size_t) q];
    return 0;
}
#endif  // WCV_NO_HOST

#endif  // WT_REGION_H_
