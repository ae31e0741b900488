// wt_text.h -- wig and bedGraph text of whole run lists (device + -DWT_EMU): the reference's writer, printBlock of
// TeeWiggleIterator (src/wigWriter.c:55-119; the parser's `write` and `write_bg`), byte for byte.  This header is the single
// source of the logic.  It is compiled
//   * by hipcc for gfx950 inside csrc/wt_text.hip (the product),
//   * by g++ with -DWT_EMU inside tests/text_emu.cpp, which runs the workgroups of every pass one after the other in any order
//     on the CPU, and as the host sweep at the end (wtx_host), and
//   * by tests/text_fmt_fuzz.cpp, which holds wtx_num against snprintf("%f").
//
// Input (the layout of wtamd_runs_histogram): n_seg segments, seg_off[n_seg + 1], start / finish / value, and a name per segment.
// The list is printed as it is given: nothing is sorted, merged or compressed.
//
// THE RULE.  The writer numbers the entries it receives from 0, across chromosomes, and prints them in blocks of WTX_ENTRIES =
// 10000 consecutive entries; every block starts out of point-by-point mode and without a previous entry, so a block is the
// unit of parallelism: ONE WORKGROUP PER BLOCK.  L = finish - start.  Without WTX_BEDGRAPH an entry is point-by-point iff the
// latest entry at or before it in its block with L < 2 or L > 5 exists and has L < 2 (wigWriter.c:69-74 as a "last setter").  A
// point-by-point entry prints L lines "%lf\n", after "fixedStep chrom=%s start=%i step=1\n" iff it is the first entry of the
// block, or the previous entry is not point-by-point, lies in another segment, or finishes before `start`.  Any other entry
// prints "%s\t%i\t%i\t%lf\n" with start - 1 and finish - 1.
//
// "%lf" IN INTEGERS (wtx_num): glibc prints the decimal expansion of the exact binary value, rounded half to even at the sixth
// decimal.  With a = |v| = m 2^sh (m < 2^53) below 2^64: ip = trunc(a) fits 64 bits; the fraction is f 2^-k with f < 2^53, so
// P = f 10^6 < 2^73 is held in two words, q = P >> k, and the k bits shifted out decide the rounding exactly; k >= 74 leaves 0;
// q == 10^6 carries into ip.  Finite |v| >= 2^64 is WIDE: the device does not print it (the door counts and refuses).
//
//   measure  validates; the mode by a last-setter scan inside the workgroup -- tiles of WTX_BLOCK entries, a lane an entry, the
//            setters of a tile as two bit masks in LDS, the mode after the tile carried in LDS --; every entry's byte count; the
//            block's total, its bad runs and its wide values
//   scan     ONE workgroup: the blocks' totals into 64-bit base offsets, in a fixed order; the three sums
//   emit     mode and byte counts again; the counts of a tile scanned in LDS; the text composed into an LDS window of WTX_WINDOW
//            bytes, which holds WTX_PIECE bytes of the tile at a time (a run may need some 450), laid out so that a window byte
//            and its address in `text` agree modulo 16: whole 16-byte lines go out as one store each, the ragged ends of a piece
//            byte by byte.  No workgroup reads `text` or writes a byte that is not its own.
#ifndef WT_TEXT_H_
#define WT_TEXT_H_

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "wt_cover.h"

#define WTX_BLOCK WCV_BLOCK
#define WTX_ENTRIES 10000                       // WTAMD_TEXT_BLOCK: the reference's BLOCK_LENGTH
#define WTX_TILES ((WTX_ENTRIES + WTX_BLOCK - 1) / WTX_BLOCK)
#define WTX_WINDOW 16384                        // bytes of the emit pass's LDS window
#define WTX_PIECE (WTX_WINDOW - 16)             // bytes of text it holds at a time (up to 15 bytes of alignment in front)
#define WTX_BEDGRAPH 1u                         // WTAMD_TEXT_BEDGRAPH
#define WTX_NAME_MAX 255

enum { WTX_K_MEASURE = 0, WTX_K_SCAN, WTX_K_EMIT, WTX_K_COUNT_ };
enum { WTX_S_BYTES = 0, WTX_S_WIDE, WTX_S_ERR, WTX_S_MODE /* after the last entry */, WTX_S_FINISH /* of the last entry */, WTX_S_N = 8 };
enum { WTX_FINITE = 0, WTX_NAN, WTX_INF, WTX_WIDE };

typedef unsigned long long wtx_u64;

struct alignas(16) WtxV4 { unsigned int x, y, z, w; };

struct alignas(16) WtxLds {
    unsigned char win[WTX_WINDOW];              // emit: the window
    wtx_u64 m1[WTX_BLOCK / 64], m0[WTX_BLOCK / 64];     // the tile's entries with L < 2 / with L > 5
    unsigned int scan[2][WTX_BLOCK];            // emit: the byte counts, scanned
    wtx_u64 acc[WTX_BLOCK];                     // measure: the lanes' bytes; scan: the lanes' slices
    unsigned int bad[WTX_BLOCK], wide[WTX_BLOCK];
    wtx_u64 tile_base;                          // emit: bytes of the block before the tile
    int carry;                                  // the mode after the tile before
};

struct WtxArgs {
    const int32_t *start, *finish;
    const void *value;
    int value_is_f64;
    long long n;                                // runs
    const int64_t *seg_off;                     // [n_seg + 1] (device)
    long long n_seg;
    const char *names;                          // the segments' names, one after the other
    const int32_t *name_off;                    // [n_seg + 1]
    unsigned int flags;
    int first;                                  // entries of workgroup 0: WTX_ENTRIES minus what the writer's open block holds
    int st_prev, st_mode, st_finish, st_same;   // workgroup 0 continues a block: the mode after, and the finish of, the entry
                                                // before; whether that entry lies in the first run's segment
    long long n_blocks;
    wtx_u64 *blk;                               // [3 n_blocks] bytes, bad runs, wide values of a block
    wtx_u64 *base;                              // [n_blocks] bytes before a block
    wtx_u64 *scalars;                           // [WTX_S_N]
    char *text;
    long long capacity;
};

// ---- "%lf" ----
struct WtxNum {
    wtx_u64 ip;                                 // integer part
    unsigned int q;                             // six decimals
    int kind, neg, nd;                          // WTX_*, the sign bit, digits of ip
};

WCV_DEV wtx_u64 wtx_mulhi(wtx_u64 a, wtx_u64 b) {
#ifdef WT_EMU
    return (wtx_u64) (((unsigned __int128) a * b) >> 64);
#else
    return __umul64hi(a, b);
#endif
}

WCV_DEV int wtx_digits(wtx_u64 x) {
    int n = 1;
    for (wtx_u64 p = 10; n < 20 && x >= p; p *= 10) n++;
    return n;
}

WCV_DEV wtx_u64 wtx_bits(double v) {
#ifdef WT_EMU
    wtx_u64 b;
    memcpy(&b, &v, 8);
    return b;
#else
    return (wtx_u64) __double_as_longlong(v);
#endif
}

WCV_DEV WtxNum wtx_num(double v) {
    const wtx_u64 b = wtx_bits(v);
    WtxNum r;
    r.neg = (int) (b >> 63); r.ip = 0; r.q = 0; r.nd = 1; r.kind = WTX_FINITE;
    int e = (int) ((b >> 52) & 0x7ff);
    wtx_u64 m = b & ((1ull << 52) - 1);
    if (e == 0x7ff) { r.kind = m ? WTX_NAN : WTX_INF; return r; }
    if (e >= 1023 + 64) { r.kind = WTX_WIDE; return r; }
    if (e) m |= 1ull << 52; else e = 1;
    const int sh = e - 1075;                    // |v| = m 2^sh
    if (sh >= 0) r.ip = m << sh;                // (sh <= 11)
    else {
        const int k = -sh;                      // 1 .. 1074
        wtx_u64 f = m;
        if (k < 64) { r.ip = m >> k; f = m & ((1ull << k) - 1); }
        if (f != 0 && k < 74) {
            const wtx_u64 lo = f * 1000000ull, hi = wtx_mulhi(f, 1000000ull);
            wtx_u64 q, rhi, rlo, hhi, hlo;      // P >> k; the k bits below; 2^(k-1)
            if (k < 64) { q = (lo >> k) | (hi << (64 - k)); rhi = 0; rlo = lo & ((1ull << k) - 1); hhi = 0; hlo = 1ull << (k - 1); }
            else if (k == 64) { q = hi; rhi = 0; rlo = lo; hhi = 0; hlo = 1ull << 63; }
            else { q = hi >> (k - 64); rhi = hi & ((1ull << (k - 64)) - 1); rlo = lo; hhi = 1ull << (k - 65); hlo = 0; }
            if (rhi > hhi || (rhi == hhi && (rlo > hlo || (rlo == hlo && (q & 1))))) q++;
            if (q == 1000000ull) { q = 0; r.ip++; }
            r.q = (unsigned int) q;
        }
    }
    r.nd = wtx_digits(r.ip);
    return r;
}

WCV_DEV unsigned int wtx_num_len(const WtxNum &n) { return (unsigned int) (n.neg + (n.kind == WTX_FINITE ? n.nd + 7 : 3)); }
WCV_DEV int wtx_digits32(unsigned int x);
WCV_DEV unsigned int wtx_int_len(long long x) { return x < 0 ? 1u + (unsigned int) wtx_digits32((unsigned int) -x) : (unsigned int) wtx_digits32((unsigned int) x); }

// ---- composing: the bytes [lo, hi) of a tile's text live at win[shift + p - lo] ----
struct WtxOut {
    unsigned char *win;
    long long lo, hi;
    int shift;
};
WCV_DEV void wtx_put(const WtxOut &o, long long p, char c) { if (p >= o.lo && p < o.hi) o.win[o.shift + (p - o.lo)] = (unsigned char) c; }
WCV_DEV long long wtx_put_str(const WtxOut &o, long long p, const char *s, int n) {
    for (int i = 0; i < n; i++) wtx_put(o, p + i, s[i]);
    return p + n;
}
WCV_DEV long long wtx_put_u64(const WtxOut &o, long long p, wtx_u64 x, int nd) {
    for (int i = nd - 1; i >= 0; i--) { wtx_put(o, p + i, (char) ('0' + (int) (x % 10))); x /= 10; }
    return p + nd;
}
// (32-bit operands divide by ten in one multiply-high of 32 bits: the coordinates, |x| <= 2^31, and the six decimals)
WCV_DEV int wtx_digits32(unsigned int x) {
    int n = 1;
    for (unsigned int p = 10; n < 10 && x >= p; p *= 10) n++;
    return n;
}
WCV_DEV long long wtx_put_u32(const WtxOut &o, long long p, unsigned int x, int nd) {
    for (int i = nd - 1; i >= 0; i--) { wtx_put(o, p + i, (char) ('0' + (int) (x % 10u))); x /= 10u; }
    return p + nd;
}
WCV_DEV long long wtx_put_int(const WtxOut &o, long long p, long long x) {
    if (x < 0) { wtx_put(o, p++, '-'); x = -x; }
    return wtx_put_u32(o, p, (unsigned int) x, wtx_digits32((unsigned int) x));
}
WCV_DEV long long wtx_put_num(const WtxOut &o, long long p, const WtxNum &n) {
    if (n.neg) wtx_put(o, p++, '-');
    if (n.kind == WTX_NAN) return wtx_put_str(o, p, "nan", 3);
    if (n.kind != WTX_FINITE) return wtx_put_str(o, p, "inf", 3);
    p = wtx_put_u64(o, p, n.ip, n.nd);
    wtx_put(o, p++, '.');
    return wtx_put_u32(o, p, n.q, 6);
}

// ---- one entry ----
struct WtxEntry {
    int32_t s, f;
    int pbp, hdr, g;                            // point-by-point; with a header; its segment
    WtxNum num;
    unsigned int bytes;
    int bad, wide;
};

WCV_DEV double wtx_value(const WtxArgs &a, long long i) {
    return a.value_is_f64 ? ((const double *) a.value)[i] : (double) ((const float *) a.value)[i];
}

// the entries of workgroup `block`: [wtx_block_first, wtx_block_end)
WCV_DEV long long wtx_block_first(const WtxArgs &a, long long block) { return block == 0 ? 0 : (long long) a.first + (block - 1) * WTX_ENTRIES; }
WCV_DEV long long wtx_block_end(const WtxArgs &a, long long block) {
    const long long e = (long long) a.first + block * WTX_ENTRIES;
    return e < a.n ? e : a.n;
}

// the mode after entry `pos` of the tile (-1: after the tile before) from the tile's masks
WCV_DEV int wtx_mode_at(const WtxLds *lds, int pos) {
    for (int w = pos >> 6; w >= 0; w--) {
        const wtx_u64 one = lds->m1[w];
        wtx_u64 any = one | lds->m0[w];
        if (w == (pos >> 6) && (pos & 63) < 63) any &= (2ull << (pos & 63)) - 1;
        if (any) return (int) ((one >> (63 - __builtin_clzll(any))) & 1ull);
    }
    return lds->carry;
}

WCV_DEV void wtx_or_lds(wtx_u64 *p, wtx_u64 v) {
#ifdef WT_EMU
    *p |= v;
#else
    atomicOr(p, v);                             // (an OR of bits in LDS: the result does not depend on the order)
#endif
}

// step A of a tile: the lanes' setters into the masks (which are zero)
WCV_DEV void wtx_tile_mark(const WtxArgs &a, long long e0, long long i1, WtxLds *lds, int l) {
    const long long i = e0 + l;
    if (i >= i1 || (a.flags & WTX_BEDGRAPH)) return;
    const long long L = (long long) a.finish[i] - (long long) a.start[i];
    if (L < 2) wtx_or_lds(&lds->m1[l >> 6], 1ull << (l & 63));
    else if (L > 5) wtx_or_lds(&lds->m0[l >> 6], 1ull << (l & 63));
}

// step B: what lane l's entry prints (the masks and the carry are complete)
WCV_DEV WtxEntry wtx_tile_entry(const WtxArgs &a, long long block, long long i0, long long e0, const WtxLds *lds, int l) {
    const long long i = e0 + l;
    WtxEntry e;
    e.s = a.start[i]; e.f = a.finish[i];
    e.num = wtx_num(wtx_value(a, i));
    e.bad = e.s >= e.f || e.s == INT32_MIN;
    e.wide = e.num.kind == WTX_WIDE;
    e.g = (int) wcv_seg_of(a.seg_off, a.n_seg, i);
    e.pbp = wtx_mode_at(lds, l);
    e.hdr = 0;
    e.bytes = 0;
    if (e.bad || e.wide) return e;
    const unsigned int nl = (unsigned int) (a.name_off[e.g + 1] - a.name_off[e.g]);
    if (e.pbp) {
        const int32_t before = a.finish[i > 0 ? i - 1 : 0];          // (loaded either way: a value to choose from, not an address)
        const bool head = i == i0, first = head && !(block == 0 && a.st_prev);
        const int pmode = head ? a.st_mode : wtx_mode_at(lds, l - 1);
        const int pfinish = head ? a.st_finish : before;
        const int psame = head ? a.st_same : (int) (i - 1 >= (long long) a.seg_off[e.g]);
        e.hdr = first || !pmode || !psame || e.s > pfinish;
        e.bytes = (e.hdr ? 31u + nl + wtx_int_len(e.s) : 0u) + (unsigned int) (e.f - e.s) * (wtx_num_len(e.num) + 1u);
    } else {
        e.bytes = nl + 1u + wtx_int_len((long long) e.s - 1) + 1u + wtx_int_len((long long) e.f - 1) + 1u + wtx_num_len(e.num) + 1u;
    }
    return e;
}

// step C (one lane): the carry for the next tile, the masks zero again
WCV_DEV void wtx_tile_close(WtxLds *lds) {
    lds->carry = wtx_mode_at(lds, WTX_BLOCK - 1);
    for (int w = 0; w < WTX_BLOCK / 64; w++) { lds->m1[w] = 0; lds->m0[w] = 0; }
}

WCV_DEV void wtx_block_open(const WtxArgs &a, long long block, WtxLds *lds) {
    lds->carry = (block == 0 && a.st_prev && !(a.flags & WTX_BEDGRAPH)) ? a.st_mode : 0;
    lds->tile_base = 0;
    for (int w = 0; w < WTX_BLOCK / 64; w++) { lds->m1[w] = 0; lds->m0[w] = 0; }
}

// ---- measure ----
WCV_DEV void wtx_measure_block(const WtxArgs &a, long long block, WtxLds *lds) {
    const long long i0 = wtx_block_first(a, block), i1 = wtx_block_end(a, block);
    WCV_LANES(l) {
        lds->acc[l] = 0; lds->bad[l] = 0; lds->wide[l] = 0;
        if (l == 0) wtx_block_open(a, block, lds);
    }
    WCV_SYNC();
    for (long long e0 = i0; e0 < i1; e0 += WTX_BLOCK) {
        WCV_LANES(l) { wtx_tile_mark(a, e0, i1, lds, l); }
        WCV_SYNC();
        WCV_LANES(l) {
            if (e0 + l < i1) {
                const WtxEntry e = wtx_tile_entry(a, block, i0, e0, lds, l);
                lds->acc[l] += e.bytes; lds->bad[l] += (unsigned int) e.bad; lds->wide[l] += (unsigned int) e.wide;
            }
        }
        WCV_SYNC();
        WCV_LANES(l) { if (l == 0) wtx_tile_close(lds); }
        WCV_SYNC();
    }
    WCV_LANES(l) {
        if (l == 0) {
            wtx_u64 bytes = 0, bad = 0, wide = 0;
            for (int k = 0; k < WTX_BLOCK; k++) { bytes += lds->acc[k]; bad += lds->bad[k]; wide += lds->wide[k]; }
            a.blk[3 * block] = bytes; a.blk[3 * block + 1] = bad; a.blk[3 * block + 2] = wide;
            if (block == a.n_blocks - 1) {
                a.scalars[WTX_S_MODE] = (wtx_u64) lds->carry;
                a.scalars[WTX_S_FINISH] = (wtx_u64) (unsigned int) a.finish[a.n - 1];
            }
        }
    }
}

// ---- scan: one workgroup, a slice per lane, the 256 slice sums by lane 0 ----
WCV_DEV void wtx_scan_block(const WtxArgs &a, long long block, WtxLds *lds) {
    if (block != 0) return;
    const long long per = (a.n_blocks + WTX_BLOCK - 1) / WTX_BLOCK;
    WCV_LANES(l) {
        wtx_u64 bytes = 0, bad = 0, wide = 0;
        for (long long b = (long long) l * per; b < (long long) (l + 1) * per && b < a.n_blocks; b++) {
            bytes += a.blk[3 * b]; bad += a.blk[3 * b + 1]; wide += a.blk[3 * b + 2];
        }
        lds->acc[l] = bytes;
        lds->bad[l] = (unsigned int) (bad > 0xffffffffull ? 0xffffffffull : bad);
        lds->wide[l] = (unsigned int) (wide > 0xffffffffull ? 0xffffffffull : wide);
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (l == 0) {
            wtx_u64 run = 0, bad = 0, wide = 0;
            for (int k = 0; k < WTX_BLOCK; k++) { const wtx_u64 c = lds->acc[k]; lds->acc[k] = run; run += c; bad += lds->bad[k]; wide += lds->wide[k]; }
            a.scalars[WTX_S_BYTES] = run; a.scalars[WTX_S_ERR] = bad; a.scalars[WTX_S_WIDE] = wide;
        }
    }
    WCV_SYNC();
    WCV_LANES(l) {
        wtx_u64 run = lds->acc[l];
        for (long long b = (long long) l * per; b < (long long) (l + 1) * per && b < a.n_blocks; b++) { a.base[b] = run; run += a.blk[3 * b]; }
    }
}

// ---- emit ----
// lane l's entry into the window
WCV_DEV void wtx_compose(const WtxArgs &a, const WtxEntry &e, const WtxOut &o, long long p) {
    const char *name = a.names + a.name_off[e.g];
    const int nl = (int) (a.name_off[e.g + 1] - a.name_off[e.g]);
    if (e.pbp) {
        if (e.hdr) {
            p = wtx_put_str(o, p, "fixedStep chrom=", 16);
            p = wtx_put_str(o, p, name, nl);
            p = wtx_put_str(o, p, " start=", 7);
            p = wtx_put_int(o, p, (long long) e.s);
            p = wtx_put_str(o, p, " step=1\n", 8);
        }
        for (int j = 0; j < e.f - e.s; j++) {
            p = wtx_put_num(o, p, e.num);
            wtx_put(o, p++, '\n');
        }
    } else {
        p = wtx_put_str(o, p, name, nl);
        wtx_put(o, p++, '\t');
        p = wtx_put_int(o, p, (long long) e.s - 1);
        wtx_put(o, p++, '\t');
        p = wtx_put_int(o, p, (long long) e.f - 1);
        wtx_put(o, p++, '\t');
        p = wtx_put_num(o, p, e.num);
        wtx_put(o, p++, '\n');
    }
}

WCV_DEV void wtx_emit_block(const WtxArgs &a, long long block, WtxLds *lds) {
    const long long i0 = wtx_block_first(a, block), i1 = wtx_block_end(a, block);
    const wtx_u64 block_base = a.base[block];
    WCV_LANES(l) { if (l == 0) wtx_block_open(a, block, lds); }
    WCV_SYNC();
    for (long long e0 = i0; e0 < i1; e0 += WTX_BLOCK) {
        WCV_LANES(l) { wtx_tile_mark(a, e0, i1, lds, l); }
        WCV_SYNC();
        WCV_LANES(l) { lds->scan[0][l] = e0 + l < i1 ? wtx_tile_entry(a, block, i0, e0, lds, l).bytes : 0u; }
        WCV_SYNC();
        int cur = 0;                            // inclusive scan of the byte counts, ending in scan[0]
        for (int d = 1; d < WTX_BLOCK; d <<= 1) {
            WCV_LANES(l) { lds->scan[cur ^ 1][l] = lds->scan[cur][l] + (l >= d ? lds->scan[cur][l - d] : 0u); }
            WCV_SYNC();
            cur ^= 1;
        }
        const long long tile_bytes = (long long) lds->scan[0][WTX_BLOCK - 1];
        const wtx_u64 tile_at = block_base + lds->tile_base;           // the tile's first byte in `text`
        for (long long p0 = 0; p0 < tile_bytes; p0 += WTX_PIECE) {
            const long long len = tile_bytes - p0 < WTX_PIECE ? tile_bytes - p0 : WTX_PIECE;
            const unsigned long long addr = (unsigned long long) (uintptr_t) a.text + tile_at + (wtx_u64) p0;
            const int shift = (int) (addr & 15ull);
            WCV_LANES(l) {
                if (e0 + l < i1) {
                    const long long end = (long long) lds->scan[0][l], beg = l ? (long long) lds->scan[0][l - 1] : 0;
                    if (beg < end && beg < p0 + len && end > p0) {
                        const WtxEntry e = wtx_tile_entry(a, block, i0, e0, lds, l);
                        const WtxOut o = {lds->win, p0, p0 + len, shift};
                        wtx_compose(a, e, o, beg);
                    }
                }
            }
            WCV_SYNC();
            WCV_LANES(l) {
                char *dst = (char *) (uintptr_t) (addr - (unsigned long long) shift);          // 16-byte aligned; window byte j <-> dst[j]
                long long total = shift + len;
                const long long room = a.capacity - (long long) (tile_at + (wtx_u64) p0) + shift;    // (never past the caller's buffer)
                if (total > room) total = room;
                for (long long c = l; c * 16 < total; c += WTX_BLOCK) {
                    const long long lo = c * 16, hi = lo + 16;
                    if (lo >= shift && hi <= total) *(WtxV4 *) (dst + lo) = *(const WtxV4 *) (lds->win + lo);
                    else for (long long j = lo < shift ? shift : lo; j < (hi < total ? hi : total); j++) dst[j] = (char) lds->win[j];
                }
            }
            WCV_SYNC();
        }
        WCV_LANES(l) { if (l == 0) { lds->tile_base += (wtx_u64) tile_bytes; wtx_tile_close(lds); } }
        WCV_SYNC();
    }
}

WCV_DEV void wtx_run_block(int kernel, const WtxArgs &a, long long block, WtxLds *lds) {
    switch (kernel) {
    case WTX_K_MEASURE: wtx_measure_block(a, block, lds); break;
    case WTX_K_SCAN: wtx_scan_block(a, block, lds); break;
    case WTX_K_EMIT: wtx_emit_block(a, block, lds); break;
    default: break;
    }
}

// the writer's state between batches (wtamd_text_state)
struct WtxState {
    int32_t in_block, point_by_point, last_finish, continues;
};

// what every entry checks before it touches anything; "" when fine
static inline const char *wtx_check(long long n_seg, const int64_t *seg_off, const char *const *seg_name, const int32_t *start, const int32_t *finish,
                                    const void *value, unsigned int flags, const WtxState *state, const void *text, long long capacity,
                                    const int64_t *n_bytes, const int64_t *n_wide) {
    if (n_seg < 0 || !seg_off || !n_bytes || !n_wide || capacity < 0 || (n_seg > 0 && !seg_name) || (capacity > 0 && !text)) return "bad argument";
    if (flags & ~WTX_BEDGRAPH) return "unknown flag";
    if (state && (state->in_block < 0 || state->in_block >= WTX_ENTRIES)) return "state: in_block outside 0 .. 9999";
    if (n_seg > 0 && seg_off[0] != 0) return "bad argument";
    for (long long g = 0; g < n_seg; g++) {
        if (seg_off[g + 1] < seg_off[g]) return "segment offsets decrease";
        if (!seg_name[g]) return "a segment without a name";
        const size_t nl = strnlen(seg_name[g], WTX_NAME_MAX + 1);
        if (nl < 1 || nl > WTX_NAME_MAX) return "a name outside 1 .. 255 bytes";
    }
    const long long n = n_seg ? (long long) seg_off[n_seg] : 0;
    if (n >= (1ll << 31) || (n > 0 && (!start || !finish || !value))) return "bad argument";
    return "";
}

// ---------------------------------------------------------------------------------------------------------------------
// The door, written once over a Launcher: the one of wt_cover.h (alloc, release, zero, to_host, to_device) with
//     bool run_text(int kernel, long long blocks, const WtxArgs &a)     and     bool sync()
// Return value: 0 fine, 1 bad argument, 2 launcher failure, 3 capacity (*n_bytes: the size needed).  Nothing is written to text
// or state unless the value is 0.  Temporary memory: 32 bytes per 10000 runs, 12 bytes and its name per segment, 64 of scalars.
// ---------------------------------------------------------------------------------------------------------------------
#ifndef WCV_NO_HOST

template <class L>
static int wtx_door(L &l, long long n_seg, const int64_t *seg_off, const char *const *seg_name, const int32_t *start, const int32_t *finish,
                    const void *value, int value_is_f64, unsigned int flags, WtxState *state, char *text, long long capacity, int64_t *n_bytes,
                    int64_t *n_wide, const char **why) {
    *why = wtx_check(n_seg, seg_off, seg_name, start, finish, value, flags, state, text, capacity, n_bytes, n_wide);
    if (**why) return 1;
    WtxArgs a = {};
    a.start = start; a.finish = finish; a.value = value; a.value_is_f64 = value_is_f64;
    a.n = n_seg ? (long long) seg_off[n_seg] : 0;
    *n_wide = 0;
    if (a.n == 0) { *n_bytes = 0; return 0; }
    a.n_seg = n_seg; a.flags = flags; a.text = text; a.capacity = capacity;
    const int in_block = state ? (int) state->in_block : 0;
    a.first = WTX_ENTRIES - in_block;
    a.st_prev = in_block > 0;
    if (a.st_prev) { a.st_mode = state->point_by_point != 0; a.st_finish = state->last_finish; a.st_same = state->continues != 0; }
    a.n_blocks = a.n <= a.first ? 1 : 1 + wcv_blocks(a.n - a.first, WTX_ENTRIES);
    std::string names;
    std::vector<int32_t> name_off((size_t) n_seg + 1, 0);
    for (long long g = 0; g < n_seg; g++) { names += seg_name[g]; name_off[(size_t) g + 1] = (int32_t) names.size(); }
    WcvScope<L> sc(l);
    int64_t *d_seg = nullptr;
    char *d_names = nullptr;
    int32_t *d_noff = nullptr;
    if (!sc.get(&d_seg, (size_t) n_seg + 1) || !sc.get(&d_names, names.size()) || !sc.get(&d_noff, (size_t) n_seg + 1) ||
        !sc.get(&a.blk, (size_t) (3 * a.n_blocks)) || !sc.get(&a.base, (size_t) a.n_blocks) || !sc.get(&a.scalars, (size_t) WTX_S_N))
        { *why = "device memory"; return 2; }
    a.seg_off = d_seg; a.names = d_names; a.name_off = d_noff;
    wtx_u64 h_sc[WTX_S_N] = {};
    if (!l.to_device(d_seg, seg_off, sizeof(int64_t) * ((size_t) n_seg + 1)) || !l.to_device(d_names, names.data(), names.size()) ||
        !l.to_device(d_noff, name_off.data(), sizeof(int32_t) * ((size_t) n_seg + 1)) || !l.zero(a.scalars, sizeof h_sc))
        { *why = "copy"; return 2; }
    if (!l.run_text(WTX_K_MEASURE, a.n_blocks, a) || !l.run_text(WTX_K_SCAN, 1, a) || !l.to_host(h_sc, a.scalars, sizeof h_sc))
        { *why = "measure pass"; return 2; }
    if (h_sc[WTX_S_ERR]) { *why = "a run with start >= finish or start == INT32_MIN"; return 1; }
    if (h_sc[WTX_S_WIDE]) { *n_wide = (int64_t) h_sc[WTX_S_WIDE]; *why = "a finite value of 2^64 or more (use the host sweep)"; return 1; }
    if (h_sc[WTX_S_BYTES] > (wtx_u64) capacity) { *n_bytes = (int64_t) h_sc[WTX_S_BYTES]; return 3; }
    if (!l.run_text(WTX_K_EMIT, a.n_blocks, a) || !l.sync()) { *why = "emit pass"; return 2; }
    *n_bytes = (int64_t) h_sc[WTX_S_BYTES];
    if (state) {
        state->in_block = (int32_t) ((in_block + a.n) % WTX_ENTRIES);
        state->point_by_point = (int32_t) h_sc[WTX_S_MODE];
        state->last_finish = (int32_t) (unsigned int) h_sc[WTX_S_FINISH];
        state->continues = 1;
    }
    return 0;
}

#endif  // WCV_NO_HOST

// The same rule on the host, without a device (a translation unit compiled with -DWT_EMU): one sweep, values through
// snprintf("%f"), so that a wide value is printed too (*n_wide counts them; they are no refusal here).  Otherwise the same
// arguments, refusals and return values as the door's, text in host memory; the same bytes.
#ifdef WT_EMU

static int wtx_host(long long n_seg, const int64_t *seg_off, const char *const *seg_name, const int32_t *start, const int32_t *finish,
                    const double *value, unsigned int flags, WtxState *state, char *text, long long capacity, int64_t *n_bytes, int64_t *n_wide) {
    if (*wtx_check(n_seg, seg_off, seg_name, start, finish, value, flags, state, text, capacity, n_bytes, n_wide)) return 1;
    const long long n = n_seg ? (long long) seg_off[n_seg] : 0;
    *n_wide = 0;
    if (n == 0) { *n_bytes = 0; return 0; }
    for (long long i = 0; i < n; i++) if (start[i] >= finish[i] || start[i] == INT32_MIN) return 1;
    WtxState st = {0, 0, 0, 0};
    if (state && state->in_block > 0) st = *state;
    const bool bed = (flags & WTX_BEDGRAPH) != 0;
    std::string out;
    char buf[400];
    long long wide = 0;
    bool fresh = true;                          // no entry of this call printed yet: `continues` decides
    for (long long g = 0; g < n_seg; g++) {
        for (long long i = seg_off[g]; i < (long long) seg_off[g + 1]; i++) {
            const bool have_prev = st.in_block > 0;
            const bool same = fresh ? st.continues != 0 : i > (long long) seg_off[g];
            const int pmode = have_prev && !bed ? st.point_by_point != 0 : 0;
            const long long L = (long long) finish[i] - (long long) start[i];
            const int mode = bed ? 0 : L < 2 ? 1 : L > 5 ? 0 : pmode;
            const double v = value[i];
            if (v - v == 0.0 && fabs(v) >= 18446744073709551616.0) wide++;
            const int nv = snprintf(buf, sizeof buf, "%f\n", v);
            if (mode) {
                if (!have_prev || !pmode || !same || start[i] > st.last_finish) {
                    out += "fixedStep chrom="; out += seg_name[g]; out += " start="; out += std::to_string(start[i]); out += " step=1\n";
                }
                for (long long j = 0; j < L; j++) out.append(buf, (size_t) nv);
            } else {
                out += seg_name[g]; out += '\t'; out += std::to_string((long long) start[i] - 1); out += '\t';
                out += std::to_string((long long) finish[i] - 1); out += '\t'; out.append(buf, (size_t) nv);
            }
            fresh = false;
            st.in_block = (st.in_block + 1) % WTX_ENTRIES;
            st.point_by_point = mode; st.last_finish = finish[i]; st.continues = 1;
        }
    }
    *n_wide = (int64_t) wide;
    if ((long long) out.size() > capacity) { *n_bytes = (int64_t) out.size(); return 3; }
    memcpy(text, out.data(), out.size());
    *n_bytes = (int64_t) out.size();
    if (state) *state = st;
    return 0;
}
#endif  // WT_EMU

#endif  // WT_TEXT_H_
