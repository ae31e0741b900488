// wt_read.h -- wig, bedGraph and BED text into run lists (device + -DWT_EMU): the inverse of wt_text.h, the reference's
// WiggleReader (src/wigReader.c) and BedReader (src/bedReader.c) over the bytes of a file.  This header is the single source of
// the rule (include/wiggletools_amd.h, wtamd_text_runs, states it).  It is compiled
//   * by hipcc for gfx950 inside csrc/wt_read.hip (the product),
//   * by g++ with -DWT_EMU inside tests/read_emu.cpp, which runs the workgroups of every pass one after the other in any order
//     on the CPU, and as the host sweep at the end (wtr_host), and
//   * by tests/read_num_fuzz.cpp, which holds wtr_number against strtod.
//
// A workgroup owns a TILE of WTR_TILE bytes; a line belongs to the tile it starts in.  Every pass over the tiles is the same
// procedure (wtr_tile): the tile's bytes into LDS as 16-byte lines, the line starts from the newlines (counts scanned in LDS),
// then rounds of WTR_BLOCK lines, a lane a line: the lane parses its line (class, integers, the number), and three scans in
// LDS give every line its data-line ordinal, its governing mode setter (a last-setter scan: a header or a bedGraph line) and
// the data line before it.  What a line needs from before its tile it takes from the tile's carry.
//   lines   per tile: lines, data lines, the last setter and the last data line (byte offsets), data lines before that setter
//   scan    ONE workgroup, fixed order: line and record bases, the last setter / data line carried into every tile
//   count   with the carry: governing header, k, coordinates; irregular lines (and the first one's offset), slow numbers,
//           segment openers, unsorted BED records per tile
//   scan2   ONE workgroup: the bases of slow numbers and segments, the totals
//   write   as count, and every record, segment and slow entry to its place (tile base + rank in LDS)
//   state   one lane: the state after the chunk, the terminal seg_off
// No atomics on global memory, no floating-point reduction: the same text gives the same bytes.  Temporary device memory:
// one WtrTile (112 bytes) per WTR_TILE bytes of text, 2 x 544 bytes of state, 128 of scalars.
//
// NUMBERS (wtr_number).  W = the digits without leading zeros and without the fraction's trailing zeros, E the decimal exponent
// that goes with it.  W == 0 is +-0; W <= 2^53 and |E| <= 22 is (double) W * 10^E or (double) W / 10^-E, ONE correctly rounded
// operation on two exact doubles (Clinger's fast path), which is strtod's result bit for bit; anything else is SLOW and left to
// the caller's strtod.  The unit is compiled without contraction; there is nothing to contract in a single operation.
#ifndef WT_READ_H_
#define WT_READ_H_

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "wt_cover.h"

#define WTR_BLOCK WCV_BLOCK
#define WTR_TILE 4096                           // bytes of text a workgroup owns (WTR_BLOCK 16-byte lines)
#define WTR_LINE_MAX 4999                       // a line of this many bytes or more is irregular (the reference's fgets(5000))
#define WTR_NAME_MAX 255
#define WTR_BED 1u                              // WTAMD_READ_BED
#define WTR_EOF 2u                              // WTAMD_READ_EOF
#define WTR_STATE_NAME (-1ll)                   // a name offset: the incoming state's chromosome
#define WTR_STATE_REC (-2ll)                    //                the incoming state's last record's name

enum { WTR_K_LINES = 0, WTR_K_SCAN, WTR_K_COUNT, WTR_K_SCAN2, WTR_K_WRITE, WTR_K_STATE, WTR_K_COUNT_ };
enum { WTR_M_BEDGRAPH = 0, WTR_M_FIXED, WTR_M_VARIABLE };
enum { WTR_L_SKIP = 0, WTR_L_FIXED, WTR_L_VARIABLE, WTR_L_DATA, WTR_L_IRREGULAR };
enum { WTR_S_LINES = 0, WTR_S_RECS, WTR_S_SEG, WTR_S_SLOW, WTR_S_IRR, WTR_S_FIRST_IRR, WTR_S_UNSORTED, WTR_S_CONTINUES, WTR_S_BAD_END,
       WTR_S_LAST_START, WTR_S_LAST_NAME_OFF, WTR_S_LAST_NAME_LEN, WTR_S_N = 16 };

typedef unsigned long long wtr_u64;

// wtamd_read_state: what one chunk of a file hands to the next; all zero at the start of a file
struct WtrState {
    int32_t mode;                               // WTR_M_*: the latest mode setter
    int32_t span, step;                         // of the latest header
    int32_t last_start;                         // of the last record
    int64_t next;                               // the start of the next fixedStep line
    int32_t chrom_len, rec_len;                 // bytes of chrom / rec_name; rec_len == 0: no record yet
    char chrom[256];                            // the latest header's chromosome
    char rec_name[256];                         // the last record's
};

// wtamd_read_counts
struct WtrCounts {
    int64_t n_lines, n_runs, n_seg, n_slow, n_irregular, first_irregular, n_unsorted, continues;
};

struct alignas(16) WtrV4 { unsigned int x, y, z, w; };

struct WtrTile {
    long long set_off, rec_off;                 // lines: byte offset of the last setter / data line that starts in the tile, -1
    long long rec_set;                          //        the setter of that data line if it starts in the tile, -1
    long long c_set, c_rec;                     // scan: the same of all the tiles before, -1
    long long b_lines, b_recs, b_slow, b_seg;   // scan, scan2: lines / data lines / slow numbers / segments before the tile
    long long first_irr;                        // count: byte offset of the tile's first irregular line, -1
    unsigned int n_lines, n_recs, set_recs;     // lines: ...; data lines of the tile before its last setter
    unsigned int rec_nf;                        //        fields of the last data line
    unsigned int n_irr, n_slow, n_seg, n_unsorted;      // count
};

struct WtrArgs {
    const unsigned char *text;
    long long n_bytes;
    unsigned int flags;
    const WtrState *st_in;                      // (device copies)
    WtrState *st_out;
    long long n_tiles;
    WtrTile *tile;
    wtr_u64 *scalars;                           // [WTR_S_N]
    int32_t *start, *finish;
    double *value;
    int64_t *seg_off, *seg_name_off;
    int32_t *seg_name_len;
    int64_t *slow_rec, *slow_off;
};

// one parsed line, as much of it as does not depend on other lines
struct WtrLine {
    long long a, b;                             // the integers of a data line
    wtr_u64 vbits;
    long long num_off, name_off;                // of the number; of the name (in wtr_tile: once the setter is known)
    int kind, nf;                               // WTR_L_*; fields of a data line (a BED line: 4)
    int name_len, slow;
    int len, pad;
};

struct WtrHdr {
    long long chrom_off, start, step, span;
    int ok, chrom_len;
};

struct alignas(16) WtrLds {
    unsigned char win[WTR_TILE + 32];           // the tile, a byte and its address in `text` agree modulo 16
    unsigned short ls[WTR_TILE];                // the line starts, relative to the tile
    WtrLine line[WTR_BLOCK];                    // the round's lines
    wtr_u64 s[2][WTR_BLOCK], b[2][WTR_BLOCK], c[2][WTR_BLOCK], f[2][WTR_BLOCK];       // the scans
    long long first[WTR_BLOCK];                 // the lanes' first irregular line
    long long n_lines;
    long long c_cnt, c_slow, c_seg, c_irr, c_uns;       // the tile's counts before the round
    wtr_u64 cb;                                 // the setter payload carried from the rounds before (0: none in the tile)
    wtr_u64 cc, cc_gov;                         // the data line carried, and its setter's payload
};

#include <locale.h>
// strtod in the "C" locale, whatever locale the embedding program has set (a ',' decimal point would read "1.5" as 1)
static inline double wtr_strtod(const char *s) {
    static locale_t c = newlocale(LC_ALL_MASK, "C", (locale_t) 0);
    return c ? strtod_l(s, nullptr, c) : strtod(s, nullptr);
}

// ---- bytes ----
struct WtrCtx {
    const unsigned char *text;
    long long n, lo, hi;                        // [lo, hi) lives in win
    const unsigned char *win;
    int shift;
};
WCV_DEV int wtr_at(const WtrCtx &c, long long p) { return (p >= c.lo && p < c.hi) ? (int) c.win[c.shift + (int) (p - c.lo)] : (int) c.text[p]; }
WCV_DEV bool wtr_sep(int ch) { return ch == ' ' || ch == '\t'; }

#ifdef WT_EMU
static const double WTR_P10[23] =
#else
__device__ const double WTR_P10[23] =
#endif
    {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

WCV_DEV wtr_u64 wtr_dbits(double v) {
#ifdef WT_EMU
    wtr_u64 b;
    memcpy(&b, &v, 8);
    return b;
#else
    return (wtr_u64) __double_as_longlong(v);
#endif
}

#define WTR_NAN_BITS 0x7ff8000000000000ull
#define WTR_INF_BITS 0x7ff0000000000000ull
#define WTR_W_MAX (1ull << 53)

// the field [p, q) as an `int`: an optional '-', then 0 or a decimal without a leading zero, inside int32
WCV_DEV bool wtr_int(const WtrCtx &c, long long p, long long q, long long *v) {
    if (p >= q) return false;
    const bool neg = wtr_at(c, p) == '-';
    if (neg) p++;
    const long long nd = q - p;
    if (nd < 1 || nd > 10) return false;
    if (wtr_at(c, p) == '0' && nd > 1) return false;
    long long x = 0;
    for (long long i = p; i < q; i++) {
        const int d = wtr_at(c, i) - '0';
        if (d < 0 || d > 9) return false;
        x = x * 10 + d;
    }
    *v = neg ? -x : x;
    return *v >= (long long) INT32_MIN && *v <= (long long) INT32_MAX;
}

// the field [p, q) as a `number`; *slow: regular, but outside the exact set (bits: NaN)
WCV_DEV bool wtr_number(const WtrCtx &c, long long p, long long q, wtr_u64 *bits, int *slow) {
    *slow = 0;
    *bits = WTR_NAN_BITS;
    if (p >= q) return false;
    const wtr_u64 neg = wtr_at(c, p) == '-' ? 1ull : 0ull;
    if (neg) p++;
    if (q - p < 1) return false;
    if (q - p == 3) {
        const int c0 = wtr_at(c, p), c1 = wtr_at(c, p + 1), c2 = wtr_at(c, p + 2);
        if (c0 == 'n' && c1 == 'a' && c2 == 'n') { *bits = WTR_NAN_BITS | (neg << 63); return true; }
        if (c0 == 'i' && c1 == 'n' && c2 == 'f') { *bits = WTR_INF_BITS | (neg << 63); return true; }
    }
    wtr_u64 W = 0;
    bool big = false, dot = false;
    long long pend = 0, fr = 0, nd_int = 0, nd_frac = 0, i = p;
    for (; i < q; i++) {
        const int ch = wtr_at(c, i);
        if (ch == '.') {
            if (dot) return false;
            dot = true;
            continue;
        }
        const int d = ch - '0';
        if (d < 0 || d > 9) break;
        if (!dot) {
            nd_int++;
            if (!big) { W = W * 10 + (wtr_u64) d; big = W > WTR_W_MAX; }
        } else {
            nd_frac++;
            if (d == 0) pend++;                 // (a trailing zero of the fraction until a digit follows)
            else if (!big) {
                if (W == 0) { fr += pend; pend = 0; }
                for (; pend > 0 && !big; pend--) { W *= 10; fr++; big = W > WTR_W_MAX; }
                if (!big) { W = W * 10 + (wtr_u64) d; fr++; big = W > WTR_W_MAX; }
                pend = 0;
            }
        }
    }
    if (nd_int + nd_frac == 0 || (dot && nd_frac == 0)) return false;
    long long ex = 0;
    if (i < q) {
        const int ch = wtr_at(c, i);
        if (ch != 'e' && ch != 'E') return false;
        i++;
        bool eneg = false;
        if (i < q && (wtr_at(c, i) == '+' || wtr_at(c, i) == '-')) { eneg = wtr_at(c, i) == '-'; i++; }
        if (q - i < 1 || q - i > 3) return false;
        for (; i < q; i++) {
            const int d = wtr_at(c, i) - '0';
            if (d < 0 || d > 9) return false;
            ex = ex * 10 + d;
        }
        if (eneg) ex = -ex;
    }
    if (big) { *slow = 1; return true; }
    if (W == 0) { *bits = neg << 63; return true; }
    const long long E = ex - fr;
    if (E < -22 || E > 22) { *slow = 1; return true; }
    const double w = (double) W;
    const double v = E >= 0 ? w * WTR_P10[E] : w / WTR_P10[-E];
    *bits = wtr_dbits(v) | (neg << 63);
    return true;
}

WCV_DEV bool wtr_starts(const WtrCtx &c, long long s, long long e, const char *kw, int n) {
    if (e - s < n) return false;
    for (int i = 0; i < n; i++) if (wtr_at(c, s + i) != kw[i]) return false;
    return true;
}

WCV_DEV bool wtr_name_ok(const WtrCtx &c, long long p, long long q, bool header) {
    if (q - p < 1 || q - p > WTR_NAME_MAX) return false;
    for (long long i = p; i < q; i++) {
        const int ch = wtr_at(c, i);
        if (ch <= 0x20 || (header && ch == '=')) return false;        // (the reference's strtok cuts a header at '=')
    }
    return true;
}

// the header line [s, e), which starts with the keyword
WCV_DEV WtrHdr wtr_header(const WtrCtx &c, long long s, long long e, bool fixed) {
    WtrHdr h;
    h.ok = 0; h.chrom_off = 0; h.chrom_len = 0; h.start = 0; h.step = 0; h.span = 1;
    int seen = 0;                               // 1 chrom, 2 start, 4 step, 8 span
    bool keeps_newline = false;
    long long p = s + (fixed ? 9 : 12);
    while (p < e) {
        if (!wtr_sep(wtr_at(c, p))) return h;
        p++;
        long long t = p, eq = -1;
        for (; t < e && !wtr_sep(wtr_at(c, t)); t++) if (eq < 0 && wtr_at(c, t) == '=') eq = t;
        if (t == p || eq < 0) return h;
        const long long kl = eq - p;
        int key = 0;
        if (kl == 5 && wtr_starts(c, p, eq, "chrom", 5)) key = 1;
        else if (kl == 5 && wtr_starts(c, p, eq, "start", 5)) key = 2;
        else if (kl == 4 && wtr_starts(c, p, eq, "step", 4)) key = 4;
        else if (kl == 4 && wtr_starts(c, p, eq, "span", 4)) key = 8;
        if (!key || (seen & key) || (!fixed && (key == 2 || key == 4))) return h;
        seen |= key;
        if (key == 1) {
            if (!wtr_name_ok(c, eq + 1, t, true)) return h;
            h.chrom_off = eq + 1; h.chrom_len = (int) (t - eq - 1);
            // (the reference cuts the line it read at " \t=" only: a chrom value that ends the line keeps the line's '\n')
            keeps_newline = t == e;
        } else {
            long long v;
            if (!wtr_int(c, eq + 1, t, &v)) return h;
            if (key == 2) h.start = v;
            else if (v < 1) return h;
            else if (key == 4) h.step = v;
            else h.span = v;
        }
        p = t;
    }
    // (After the loop, not as `if (t == e && e < c.n) h.chrom_len++;` inside the `key == 1` branch: with that form AMD clang 22.0.0git
    // of ROCm 7.2.0 (HIP 7.2.26015) stops at -O3 for gfx950 with "Illegal instruction detected: Operand has incorrect register
    // class. V_CMP_NE_U32_e32 0, $src_shared_base" while compiling wt_read_kernel; this form compiles.)
    if (keeps_newline && e < c.n) h.chrom_len++;
    h.ok = (fixed ? (seen & 7) == 7 : (seen & 1) == 1) && h.chrom_len <= WTR_NAME_MAX;
    return h;
}

// the end of the line that starts at s: its '\n', n_bytes, or s + WTR_LINE_MAX (irregular, whatever follows)
WCV_DEV long long wtr_line_end(const WtrCtx &c, long long s) {
    long long e = s;
    const long long stop = s + WTR_LINE_MAX < c.n ? s + WTR_LINE_MAX : c.n;
    while (e < stop && wtr_at(c, e) != '\n') e++;
    return e;
}

// the maximal [-]digits at p (inside [p, e)) as an `int`; *q: where it ends
WCV_DEV bool wtr_int_prefix(const WtrCtx &c, long long p, long long e, long long *v, long long *q) {
    long long t = p;
    if (t < e && wtr_at(c, t) == '-') t++;
    while (t < e && wtr_at(c, t) >= '0' && wtr_at(c, t) <= '9') t++;
    *q = t;
    return wtr_int(c, p, t, v);
}

// the head of a BED line [s, e): name, blanks, int
WCV_DEV bool wtr_bed_head(const WtrCtx &c, long long s, long long e, int *name_len, long long *a, long long *q) {
    long long p = s;
    while (p < e && wtr_at(c, p) > 0x20) p++;
    if (p - s < 1 || p - s > WTR_NAME_MAX) return false;
    *name_len = (int) (p - s);
    long long t = p;
    while (t < e && wtr_sep(wtr_at(c, t))) t++;
    if (t == p) return false;
    return wtr_int_prefix(c, t, e, a, q);
}

// the line [s, e) (e - s < WTR_LINE_MAX)
WCV_DEV WtrLine wtr_parse(const WtrCtx &c, long long s, long long e, unsigned int flags) {
    WtrLine ln;
    ln.a = 0; ln.b = 0; ln.vbits = WTR_NAN_BITS; ln.num_off = s; ln.name_off = s; ln.kind = WTR_L_IRREGULAR; ln.nf = 0; ln.name_len = 0; ln.slow = 0;
    ln.len = (int) (e - s); ln.pad = 0;
    if (e == s) return ln;
    if (wtr_at(c, s) == '#') { ln.kind = WTR_L_SKIP; return ln; }
    if (flags & WTR_BED) {
        for (long long p = s; p < e; p++) if (wtr_at(c, p) == '\r') return ln;
        long long q, t;
        if (!wtr_bed_head(c, s, e, &ln.name_len, &ln.a, &q)) return ln;
        for (t = q; t < e && wtr_sep(wtr_at(c, t)); t++) { }
        if (t == q || !wtr_int_prefix(c, t, e, &ln.b, &q)) return ln;
        if (ln.b == 0 && q < e && (wtr_at(c, q) == 'x' || wtr_at(c, q) == 'X')) return ln;       // (the reference's %i reads on)
        if (ln.a >= (long long) INT32_MAX || ln.b >= (long long) INT32_MAX) return ln;
        ln.vbits = 0x3ff0000000000000ull;
        ln.nf = 4; ln.kind = WTR_L_DATA;
        return ln;
    }
    if (wtr_starts(c, s, e, "track", 5)) { ln.kind = WTR_L_SKIP; return ln; }
    if (wtr_starts(c, s, e, "variableStep", 12)) { if (wtr_header(c, s, e, false).ok) ln.kind = WTR_L_VARIABLE; return ln; }
    if (wtr_starts(c, s, e, "fixedStep", 9)) { if (wtr_header(c, s, e, true).ok) ln.kind = WTR_L_FIXED; return ln; }
    long long sp[3] = {e, e, e};
    int nsep = 0;
    for (long long p = s; p < e; p++) {
        const int ch = wtr_at(c, p);
        if (ch == '\r') return ln;
        if (wtr_sep(ch)) {
            if (nsep == 0) sp[0] = p; else if (nsep == 1) sp[1] = p; else if (nsep == 2) sp[2] = p;
            nsep++;
        }
    }
    long long num = s;
    if (nsep == 3) {
        if (!wtr_name_ok(c, s, sp[0], false)) return ln;
        ln.name_len = (int) (sp[0] - s);
        if (!wtr_int(c, sp[0] + 1, sp[1], &ln.a) || !wtr_int(c, sp[1] + 1, sp[2], &ln.b)) return ln;
        if (ln.a >= (long long) INT32_MAX || ln.b >= (long long) INT32_MAX) return ln;
        num = sp[2] + 1;
    } else if (nsep == 1) {
        if (!wtr_int(c, s, sp[0], &ln.a)) return ln;
        num = sp[0] + 1;
    } else if (nsep != 0) return ln;
    if (!wtr_number(c, num, e, &ln.vbits, &ln.slow)) return ln;
    ln.num_off = num;
    ln.nf = nsep + 1; ln.kind = WTR_L_DATA;
    return ln;
}

// ---- names: (offset in text | WTR_STATE_NAME | WTR_STATE_REC, length) ----
WCV_DEV int wtr_name_byte(const WtrArgs &a, const WtrCtx &c, long long off, int i) {
    if (off == WTR_STATE_NAME) return (int) (unsigned char) a.st_in->chrom[i];
    if (off == WTR_STATE_REC) return (int) (unsigned char) a.st_in->rec_name[i];
    return wtr_at(c, off + i);
}
WCV_DEV bool wtr_same_name(const WtrArgs &a, const WtrCtx &c, long long o1, int l1, long long o2, int l2) {
    if (l1 != l2) return false;
    if (o1 == o2) return true;
    for (int i = 0; i < l1; i++) if (wtr_name_byte(a, c, o1, i) != wtr_name_byte(a, c, o2, i)) return false;
    return true;
}
// strcmp of two names: < 0, 0, > 0
WCV_DEV int wtr_cmp_name(const WtrArgs &a, const WtrCtx &c, long long o1, int l1, long long o2, int l2) {
    for (int i = 0; i < l1 && i < l2; i++) {
        const int d = wtr_name_byte(a, c, o1, i) - wtr_name_byte(a, c, o2, i);
        if (d) return d;
    }
    return l1 - l2;
}

// what governs the lines after the setter at byte offset H (-1: the state)
struct WtrGov {
    int mode, chrom_len;
    long long chrom_off, start, step, span;
    long long S;                                // data lines of the chunk before it
};
WCV_DEV WtrGov wtr_gov(const WtrArgs &a, const WtrCtx &c, long long H, long long S) {
    WtrGov g;
    g.S = S;
    if (H < 0) {
        g.mode = a.st_in->mode; g.chrom_off = WTR_STATE_NAME; g.chrom_len = a.st_in->chrom_len;
        g.start = a.st_in->next; g.step = a.st_in->step; g.span = a.st_in->span; g.S = 0;
        return g;
    }
    const long long e = wtr_line_end(c, H);
    const bool fixed = wtr_at(c, H) == 'f' && wtr_starts(c, H, e, "fixedStep", 9), var = !fixed && wtr_starts(c, H, e, "variableStep", 12);
    g.mode = WTR_M_BEDGRAPH; g.chrom_off = H; g.chrom_len = 0; g.start = 0; g.step = 0; g.span = 0;
    if (fixed || var) {
        const WtrHdr h = wtr_header(c, H, e, fixed);
        g.mode = fixed ? WTR_M_FIXED : WTR_M_VARIABLE; g.chrom_off = h.chrom_off; g.chrom_len = h.chrom_len;
        g.start = h.start; g.step = h.step; g.span = h.span;
    }
    return g;
}
// data lines of the chunk before the setter H of an EARLIER tile (the last setter of its tile)
WCV_DEV long long wtr_S_of(const WtrArgs &a, long long H) {
    if (H < 0) return 0;
    const WtrTile &t = a.tile[H / WTR_TILE];
    return t.b_recs + (long long) t.set_recs;
}

// inclusive scans over the lanes (Hillis-Steele, ending in buffer 0); identity 0
WCV_DEV void wtr_scan_sum(wtr_u64 (*buf)[WTR_BLOCK]) {
    int cur = 0;
    for (int d = 1; d < WTR_BLOCK; d <<= 1) {
        WCV_LANES(l) { buf[cur ^ 1][l] = buf[cur][l] + (l >= d ? buf[cur][l - d] : 0ull); }
        WCV_SYNC();
        cur ^= 1;
    }
}
WCV_DEV void wtr_scan_max2(wtr_u64 (*b1)[WTR_BLOCK], wtr_u64 (*b2)[WTR_BLOCK]) {
    int cur = 0;
    for (int d = 1; d < WTR_BLOCK; d <<= 1) {
        WCV_LANES(l) {
            const wtr_u64 x1 = b1[cur][l], y1 = l >= d ? b1[cur][l - d] : 0ull, x2 = b2[cur][l], y2 = l >= d ? b2[cur][l - d] : 0ull;
            b1[cur ^ 1][l] = x1 > y1 ? x1 : y1;
            b2[cur ^ 1][l] = x2 > y2 ? x2 : y2;
        }
        WCV_SYNC();
        cur ^= 1;
    }
}

// payloads of the max scans.  A setter: (offset in the tile + 1) << 13 | data lines of the tile before it.
// A data line: (offset in the tile + 1) << 11 | lane << 3 | fields.
WCV_DEV long long wtr_pay_off(wtr_u64 pay, int sh) { return (long long) (pay >> sh) - 1; }

// ---- a tile, in pass `pass` (WTR_K_LINES, WTR_K_COUNT, WTR_K_WRITE) ----
WCV_DEV void wtr_tile(int pass, const WtrArgs &a, long long t, WtrLds *lds) {
    const long long lo = t * WTR_TILE, hi = lo + WTR_TILE < a.n_bytes ? lo + WTR_TILE : a.n_bytes;
    const unsigned long long addr = (unsigned long long) (uintptr_t) a.text + (unsigned long long) lo;
    const int shift = (int) (addr & 15ull);
    WtrCtx c;
    c.text = a.text; c.n = a.n_bytes; c.lo = lo; c.hi = hi; c.win = lds->win; c.shift = shift;
    // the tile into LDS: whole 16-byte lines where all 16 bytes are text, byte by byte at the ragged ends
    WCV_LANES(l) {
        const unsigned char *base = (const unsigned char *) (uintptr_t) (addr - (unsigned long long) shift);     // window byte j <-> base[j]
        const long long total = shift + (hi - lo);
        for (long long v = l; v * 16 < total; v += WTR_BLOCK) {
            const long long b0 = v * 16, b1 = b0 + 16;
            if (b0 >= shift && b1 <= total) *(WtrV4 *) (lds->win + b0) = *(const WtrV4 *) (base + b0);
            else for (long long j = b0 < shift ? shift : b0; j < (b1 < total ? b1 : total); j++) lds->win[j] = base[j];
        }
        lds->first[l] = -1;
        if (l == 0) { lds->c_cnt = 0; lds->c_slow = 0; lds->c_seg = 0; lds->c_irr = 0; lds->c_uns = 0; lds->cb = 0; lds->cc = 0; lds->cc_gov = 0; }
    }
    WCV_SYNC();
    // the line starts: p == 0, or the byte before p is '\n'
    WCV_LANES(l) {
        unsigned int n = 0;
        for (int i = 0; i < 16; i++) {
            const long long p = lo + (long long) l * 16 + i;
            if (p < hi && (p == 0 || wtr_at(c, p - 1) == '\n')) n++;
        }
        lds->s[0][l] = n;
    }
    WCV_SYNC();
    wtr_scan_sum(lds->s);
    WCV_LANES(l) {
        unsigned int k = (unsigned int) lds->s[0][l];
        for (int i = 15; i >= 0; i--) {
            const long long p = lo + (long long) l * 16 + i;
            if (p < hi && (p == 0 || wtr_at(c, p - 1) == '\n')) lds->ls[--k] = (unsigned short) (p - lo);
        }
        if (l == WTR_BLOCK - 1) lds->n_lines = (long long) lds->s[0][l];
    }
    WCV_SYNC();
    const long long n_lines = lds->n_lines;
    const WtrTile me = a.tile[t];               // (the fields of the passes before)
    const long long n_recs_all = pass == WTR_K_WRITE ? (long long) a.scalars[WTR_S_RECS] : 0;
    for (long long r0 = 0; r0 < n_lines; r0 += WTR_BLOCK) {
        // the lane's line, by itself
        WCV_LANES(l) {
            const long long j = r0 + l;
            wtr_u64 ps = 0, pc = 0;
            if (j < n_lines) {
                const long long s = lo + (long long) lds->ls[j];
                const long long e = j + 1 < n_lines ? lo + (long long) lds->ls[j + 1] - 1 : wtr_line_end(c, s);
                const WtrLine ln = wtr_parse(c, s, e - s >= WTR_LINE_MAX ? s : e, a.flags);    // (too long: irregular as an empty line is)
                lds->line[l] = ln;
                if (ln.kind == WTR_L_DATA) {
                    ps = 1ull | ((wtr_u64) ln.slow << 16);
                    pc = ((wtr_u64) (s - lo + 1) << 11) | ((wtr_u64) l << 3) | (wtr_u64) ln.nf;
                }
            }
            lds->s[0][l] = ps; lds->c[0][l] = pc;
        }
        WCV_SYNC();
        wtr_scan_sum(lds->s);
        // the setters, with the data lines of the tile before them
        WCV_LANES(l) {
            const long long j = r0 + l;
            wtr_u64 pb = 0;
            if (j < n_lines && !(a.flags & WTR_BED)) {
                const int kind = lds->line[l].kind, nf = lds->line[l].nf;
                const bool setter = kind == WTR_L_FIXED || kind == WTR_L_VARIABLE || (kind == WTR_L_DATA && nf == 4);
                const wtr_u64 before = (wtr_u64) lds->c_cnt + (lds->s[0][l] & 0xffffull) - (kind == WTR_L_DATA ? 1ull : 0ull);
                if (setter) pb = ((wtr_u64) ((long long) lds->ls[j] + 1) << 13) | before;
            }
            lds->b[0][l] = pb;
        }
        WCV_SYNC();
        wtr_scan_max2(lds->b, lds->c);
        // the line among the others
        WCV_LANES(l) {
            const long long j = r0 + l;
            wtr_u64 flags3 = 0;                 // opens a segment | irregular << 16 | unsorted << 32
            if (j < n_lines && pass != WTR_K_LINES) {
                const WtrLine ln = lds->line[l];
                const long long s = lo + (long long) lds->ls[j];
                bool irregular = ln.kind == WTR_L_IRREGULAR;
                if (ln.kind == WTR_L_DATA) {
                    const long long R = me.b_recs + lds->c_cnt + (long long) (lds->s[0][l] & 0xffffull) - 1;      // its ordinal in the chunk
                    // its setter: of this round, of the rounds before, of the tiles before (an inclusive scan: a bedGraph line is its own)
                    const wtr_u64 gb = lds->b[0][l] ? lds->b[0][l] : lds->cb;
                    const long long H = gb ? lo + wtr_pay_off(gb, 13) : me.c_set;
                    // the data line before it, and that line's setter
                    const wtr_u64 pc = l > 0 ? lds->c[0][l - 1] : 0ull;
                    long long P, PH;
                    int pnf;
                    if (pc) {
                        const int lp = (int) ((pc >> 3) & 255ull);
                        const wtr_u64 pg = lds->b[0][lp] ? lds->b[0][lp] : lds->cb;
                        P = lo + wtr_pay_off(pc, 11); pnf = (int) (pc & 7ull); PH = pg ? lo + wtr_pay_off(pg, 13) : me.c_set;
                    } else if (lds->cc) {
                        P = lo + wtr_pay_off(lds->cc, 11); pnf = (int) (lds->cc & 7ull); PH = lds->cc_gov ? lo + wtr_pay_off(lds->cc_gov, 13) : me.c_set;
                    } else {
                        P = me.c_rec; pnf = 0; PH = -1;
                        if (P >= 0) {
                            const WtrTile &tp = a.tile[P / WTR_TILE];
                            pnf = (int) tp.rec_nf; PH = tp.rec_set >= 0 ? tp.rec_set : tp.c_set;
                        }
                    }
                    long long name_off = s, start = ln.a + 1, finish = ln.b + 1;
                    int name_len = ln.name_len;
                    bool compare = true;                // its name with the one before: a line under a header only right after that header
                    if (ln.nf != 4) {
                        const WtrGov g = wtr_gov(a, c, H, gb ? me.b_recs + (long long) (gb & 8191ull) : wtr_S_of(a, H));
                        name_off = g.chrom_off; name_len = g.chrom_len;
                        if (ln.nf == 2) {
                            irregular = g.mode != WTR_M_VARIABLE;
                            start = ln.a; finish = ln.a + g.span;
                        } else {
                            irregular = g.mode != WTR_M_FIXED;
                            start = g.start + (R - g.S) * g.step; finish = start + g.span;
                        }
                        if (start > (long long) INT32_MAX || finish > (long long) INT32_MAX || start < (long long) INT32_MIN) irregular = true;
                        compare = P < H || P < 0;
                    }
                    // does it open a segment?  is a BED record before its predecessor?
                    bool opens = R == 0, unsorted = false;
                    if (!irregular && compare) {
                        long long pn_off = P, pstart = 0;
                        int pn_len = 0;
                        bool have = true;
                        if (P < 0) {
                            pn_off = WTR_STATE_REC; pn_len = a.st_in->rec_len; pstart = a.st_in->last_start; have = pn_len > 0;
                        } else if (a.flags & WTR_BED) {
                            long long q;
                            (void) wtr_bed_head(c, P, wtr_line_end(c, P), &pn_len, &pstart, &q);
                            pstart++;
                        } else if (pnf == 4) {
                            while (pn_len <= WTR_NAME_MAX && !wtr_sep(wtr_at(c, P + pn_len))) pn_len++;
                        } else {
                            const WtrGov pg = wtr_gov(a, c, PH, 0);
                            pn_off = pg.chrom_off; pn_len = pg.chrom_len;
                        }
                        const bool same = have && wtr_same_name(a, c, name_off, name_len, pn_off, pn_len);
                        if (!same) opens = true;
                        if (have && (a.flags & WTR_BED)) {
                            const int d = wtr_cmp_name(a, c, name_off, name_len, pn_off, pn_len);
                            unsorted = d < 0 || (d == 0 && start < pstart);
                        }
                        if (R == 0 && pass == WTR_K_COUNT) a.scalars[WTR_S_CONTINUES] = same ? 1ull : 0ull;
                    }
                    if (irregular) opens = false;
                    flags3 = (opens ? 1ull : 0ull) | (unsorted ? 1ull << 32 : 0ull);
                    if (pass == WTR_K_WRITE) {
                        a.start[R] = (int32_t) start; a.finish[R] = (int32_t) finish;
                        ((wtr_u64 *) a.value)[R] = ln.vbits;
                        if (R == n_recs_all - 1) {
                            a.scalars[WTR_S_LAST_START] = (wtr_u64) start; a.scalars[WTR_S_LAST_NAME_OFF] = (wtr_u64) name_off;
                            a.scalars[WTR_S_LAST_NAME_LEN] = (wtr_u64) name_len;
                        }
                    }
                    lds->line[l].name_off = name_off; lds->line[l].name_len = name_len;      // (for the placing below)
                }
                if (irregular) {
                    flags3 |= 1ull << 16;
                    if (lds->first[l] < 0) lds->first[l] = s;
                }
            }
            lds->f[0][l] = flags3;
        }
        WCV_SYNC();
        wtr_scan_sum(lds->f);
        if (pass == WTR_K_WRITE) {
            WCV_LANES(l) {
                const long long j = r0 + l;
                if (j < n_lines && lds->line[l].kind == WTR_L_DATA) {
                    const WtrLine &ln = lds->line[l];
                    const long long R = me.b_recs + lds->c_cnt + (long long) (lds->s[0][l] & 0xffffull) - 1;
                    const wtr_u64 incl = lds->f[0][l] & 0xffffull, excl = l > 0 ? lds->f[0][l - 1] & 0xffffull : 0ull;
                    if (incl != excl) {
                        const long long g = me.b_seg + lds->c_seg + (long long) excl;
                        a.seg_off[g] = R; a.seg_name_off[g] = ln.name_off; a.seg_name_len[g] = ln.name_len;
                    }
                    if (ln.slow) {
                        const long long k = me.b_slow + lds->c_slow + (long long) ((lds->s[0][l] >> 16) & 0xffffull) - 1;
                        a.slow_rec[k] = R; a.slow_off[k] = ln.num_off;
                    }
                }
            }
        }
        WCV_SYNC();
        // the carries for the next round, by one lane
        WCV_LANES(l) {
            if (l == WTR_BLOCK - 1) {
                const wtr_u64 tot = lds->s[0][l], f3 = lds->f[0][l], lastc = lds->c[0][l], lastb = lds->b[0][l];
                lds->c_cnt += (long long) (tot & 0xffffull); lds->c_slow += (long long) ((tot >> 16) & 0xffffull);
                lds->c_seg += (long long) (f3 & 0xffffull); lds->c_irr += (long long) ((f3 >> 16) & 0xffffull); lds->c_uns += (long long) ((f3 >> 32) & 0xffffull);
                if (lastc) {
                    const int lp = (int) ((lastc >> 3) & 255ull);
                    lds->cc_gov = lds->b[0][lp] ? lds->b[0][lp] : lds->cb;
                    lds->cc = lastc;
                }
                if (lastb) lds->cb = lastb;
            }
        }
        WCV_SYNC();
    }
    // what the tile hands on
    WCV_LANES(l) {
        if (l == 0) {
            WtrTile &o = a.tile[t];
            if (pass == WTR_K_LINES) {
                o.set_off = lds->cb ? lo + wtr_pay_off(lds->cb, 13) : -1; o.set_recs = (unsigned int) (lds->cb & 8191ull);
                o.rec_off = lds->cc ? lo + wtr_pay_off(lds->cc, 11) : -1; o.rec_nf = (unsigned int) (lds->cc & 7ull);
                o.rec_set = lds->cc && lds->cc_gov ? lo + wtr_pay_off(lds->cc_gov, 13) : -1;
                o.n_lines = (unsigned int) n_lines; o.n_recs = (unsigned int) lds->c_cnt;
                if (t == a.n_tiles - 1) a.scalars[WTR_S_BAD_END] = (a.text[a.n_bytes - 1] != '\n' && !(a.flags & WTR_EOF)) ? 1ull : 0ull;
            } else if (pass == WTR_K_COUNT) {
                long long first = -1;
                for (int k = 0; k < WTR_BLOCK; k++) if (lds->first[k] >= 0 && (first < 0 || lds->first[k] < first)) first = lds->first[k];
                o.first_irr = first; o.n_irr = (unsigned int) lds->c_irr; o.n_slow = (unsigned int) lds->c_slow; o.n_seg = (unsigned int) lds->c_seg;
                o.n_unsorted = (unsigned int) lds->c_uns;
            }
        }
    }
}

// ---- scan / scan2: ONE workgroup, a slice of the tiles per lane, the 256 slices by lane 0; a fixed order ----
WCV_DEV void wtr_scan_tiles(int pass, const WtrArgs &a, long long block, WtrLds *lds) {
    if (block != 0) return;
    const bool first = pass == WTR_K_SCAN;
    const long long per = (a.n_tiles + WTR_BLOCK - 1) / WTR_BLOCK;
    long long *mx = (long long *) lds->c[0], *my = (long long *) lds->c[1], *fi = lds->first;
    WCV_LANES(l) {
        wtr_u64 x = 0, y = 0, z = 0, w = 0;
        long long m1 = -1, m2 = -1, f = -1;
        for (long long t = (long long) l * per; t < (long long) (l + 1) * per && t < a.n_tiles; t++) {
            const WtrTile &o = a.tile[t];
            if (first) {
                x += o.n_lines; y += o.n_recs;
                if (o.set_off > m1) m1 = o.set_off;
                if (o.rec_off > m2) m2 = o.rec_off;
            } else {
                x += o.n_slow; y += o.n_seg; z += o.n_irr; w += o.n_unsorted;
                if (f < 0) f = o.first_irr;
            }
        }
        lds->s[0][l] = x; lds->s[1][l] = y; lds->b[0][l] = z; lds->b[1][l] = w; mx[l] = m1; my[l] = m2; fi[l] = f;
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (l == 0) {
            wtr_u64 x = 0, y = 0, z = 0, w = 0;
            long long m1 = -1, m2 = -1, f = -1;
            for (int k = 0; k < WTR_BLOCK; k++) {
                const wtr_u64 cx = lds->s[0][k], cy = lds->s[1][k];
                const long long c1 = mx[k], c2 = my[k];
                lds->s[0][k] = x; lds->s[1][k] = y; mx[k] = m1; my[k] = m2;
                x += cx; y += cy; z += lds->b[0][k]; w += lds->b[1][k];
                if (c1 > m1) m1 = c1;
                if (c2 > m2) m2 = c2;
                if (f < 0) f = fi[k];
            }
            if (first) { a.scalars[WTR_S_LINES] = x; a.scalars[WTR_S_RECS] = y; }
            else {
                a.scalars[WTR_S_SLOW] = x; a.scalars[WTR_S_SEG] = y; a.scalars[WTR_S_IRR] = z; a.scalars[WTR_S_UNSORTED] = w;
                a.scalars[WTR_S_FIRST_IRR] = (wtr_u64) f;
            }
        }
    }
    WCV_SYNC();
    WCV_LANES(l) {
        wtr_u64 x = lds->s[0][l], y = lds->s[1][l];
        long long m1 = mx[l], m2 = my[l];
        for (long long t = (long long) l * per; t < (long long) (l + 1) * per && t < a.n_tiles; t++) {
            WtrTile &o = a.tile[t];
            if (first) {
                o.b_lines = (long long) x; o.b_recs = (long long) y; o.c_set = m1; o.c_rec = m2;
                x += o.n_lines; y += o.n_recs;
                if (o.set_off > m1) m1 = o.set_off;
                if (o.rec_off > m2) m2 = o.rec_off;
            } else {
                o.b_slow = (long long) x; o.b_seg = (long long) y;
                x += o.n_slow; y += o.n_seg;
            }
        }
    }
}

// ---- state: one lane writes the state after the chunk and the terminal seg_off ----
WCV_DEV void wtr_state_block(const WtrArgs &a, long long block, WtrLds *) {
    if (block != 0) return;
    WCV_LANES(l) {
        if (l == 0) {
            WtrCtx c;
            c.text = a.text; c.n = a.n_bytes; c.lo = 0; c.hi = 0; c.win = nullptr; c.shift = 0;
            const WtrTile &z = a.tile[a.n_tiles - 1];
            const long long H = z.set_off > z.c_set ? z.set_off : z.c_set;
            const long long n_recs = (long long) a.scalars[WTR_S_RECS], n_seg = (long long) a.scalars[WTR_S_SEG];
            WtrState *o = a.st_out;
            const WtrState *in = a.st_in;
            o->mode = in->mode; o->span = in->span; o->step = in->step; o->last_start = in->last_start; o->next = in->next;
            o->chrom_len = in->chrom_len; o->rec_len = in->rec_len;
            for (int i = 0; i < 256; i++) { o->chrom[i] = in->chrom[i]; o->rec_name[i] = in->rec_name[i]; }
            if (!(a.flags & WTR_BED)) {
                if (H < 0) {
                    if (in->mode == WTR_M_FIXED) o->next = in->next + n_recs * (long long) in->step;
                } else {
                    const WtrGov g = wtr_gov(a, c, H, H == z.set_off ? z.b_recs + (long long) z.set_recs : wtr_S_of(a, H));
                    o->mode = g.mode; o->span = (int32_t) g.span; o->step = (int32_t) g.step;
                    o->next = g.mode == WTR_M_FIXED ? g.start + (n_recs - g.S) * g.step : 0;
                    o->chrom_len = g.mode == WTR_M_BEDGRAPH ? 0 : g.chrom_len;
                    for (int i = 0; i < 256; i++) o->chrom[i] = i < o->chrom_len ? (char) wtr_at(c, g.chrom_off + i) : (char) 0;
                }
            }
            if (n_recs > 0) {
                const long long off = (long long) a.scalars[WTR_S_LAST_NAME_OFF];
                const int len = (int) a.scalars[WTR_S_LAST_NAME_LEN];
                o->last_start = (int32_t) (long long) a.scalars[WTR_S_LAST_START];
                o->rec_len = len;
                for (int i = 0; i < 256; i++) o->rec_name[i] = i < len ? (char) wtr_name_byte(a, c, off, i) : (char) 0;
                a.seg_off[n_seg] = n_recs;
            }
        }
    }
}

WCV_DEV void wtr_run_block(int kernel, const WtrArgs &a, long long block, WtrLds *lds) {
    switch (kernel) {
    case WTR_K_LINES: wtr_tile(WTR_K_LINES, a, block, lds); break;
    case WTR_K_SCAN: wtr_scan_tiles(WTR_K_SCAN, a, block, lds); break;
    case WTR_K_COUNT: wtr_tile(WTR_K_COUNT, a, block, lds); break;
    case WTR_K_SCAN2: wtr_scan_tiles(WTR_K_SCAN2, a, block, lds); break;
    case WTR_K_WRITE: wtr_tile(WTR_K_WRITE, a, block, lds); break;
    case WTR_K_STATE: wtr_state_block(a, block, lds); break;
    default: break;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The door, written once over a Launcher: the one of wt_cover.h (alloc, release, zero, to_host, to_device) with
//     bool run_read(int kernel, long long blocks, const WtrArgs &a)     and     bool sync()
// text and the output arrays are DEVICE memory, state and counts HOST.  Return value: 0 fine, 1 bad argument or irregular /
// unsorted text, 2 launcher failure, 3 capacity.  counts is written whenever the text was looked at; the output arrays and the
// state only when the value is 0.  seg_off holds seg_capacity + 1 entries: seg_off[n_seg] = n_runs.
// ---------------------------------------------------------------------------------------------------------------------
#ifndef WCV_NO_HOST

template <class L>
static int wtr_door(L &l, const char *text, long long n_bytes, unsigned int flags, WtrState *state, int32_t *start, int32_t *finish, double *value,
                    long long capacity, int64_t *seg_off, int64_t *seg_name_off, int32_t *seg_name_len, long long seg_capacity, int64_t *slow_rec,
                    int64_t *slow_off, long long slow_capacity, WtrCounts *counts, const char **why) {
    *why = "";
    if (!state || !counts || n_bytes < 0 || capacity < 0 || seg_capacity < 0 || slow_capacity < 0 || (n_bytes > 0 && !text)) { *why = "bad argument"; return 1; }
    if (flags & ~(WTR_BED | WTR_EOF)) { *why = "unknown flag"; return 1; }
    if ((capacity > 0 && (!start || !finish || !value)) || (seg_capacity > 0 && (!seg_off || !seg_name_off || !seg_name_len)) ||
        (slow_capacity > 0 && (!slow_rec || !slow_off))) { *why = "bad argument"; return 1; }
    if (state->mode < WTR_M_BEDGRAPH || state->mode > WTR_M_VARIABLE || state->chrom_len < 0 || state->chrom_len > WTR_NAME_MAX || state->rec_len < 0 ||
        state->rec_len > WTR_NAME_MAX) { *why = "state: not one this door wrote"; return 1; }
    if (n_bytes >= (1ll << 40)) { *why = "more than 2^40 bytes"; return 1; }
    WtrCounts cn = {};
    cn.first_irregular = -1;
    if (n_bytes == 0) { *counts = cn; return 0; }
    WtrArgs a = {};
    a.text = (const unsigned char *) text; a.n_bytes = n_bytes; a.flags = flags;
    a.n_tiles = wcv_blocks(n_bytes, WTR_TILE);
    a.start = start; a.finish = finish; a.value = value; a.seg_off = seg_off; a.seg_name_off = seg_name_off; a.seg_name_len = seg_name_len;
    a.slow_rec = slow_rec; a.slow_off = slow_off;
    WcvScope<L> sc(l);
    WtrState *d_in = nullptr;
    if (!sc.get(&d_in, 1) || !sc.get(&a.st_out, 1) || !sc.get(&a.tile, (size_t) a.n_tiles) || !sc.get(&a.scalars, (size_t) WTR_S_N)) { *why = "device memory"; return 2; }
    a.st_in = d_in;
    wtr_u64 h[WTR_S_N] = {};
    if (!l.to_device(d_in, state, sizeof(WtrState)) || !l.zero(a.scalars, sizeof h)) { *why = "copy"; return 2; }
    if (!l.run_read(WTR_K_LINES, a.n_tiles, a) || !l.run_read(WTR_K_SCAN, 1, a) || !l.run_read(WTR_K_COUNT, a.n_tiles, a) ||
        !l.run_read(WTR_K_SCAN2, 1, a) || !l.to_host(h, a.scalars, sizeof h)) { *why = "count passes"; return 2; }
    if (h[WTR_S_BAD_END]) { *why = "the text does not end in a newline (WTAMD_READ_EOF allows a file's last line)"; return 1; }
    cn.n_lines = (int64_t) h[WTR_S_LINES]; cn.n_runs = (int64_t) h[WTR_S_RECS]; cn.n_seg = (int64_t) h[WTR_S_SEG]; cn.n_slow = (int64_t) h[WTR_S_SLOW];
    cn.n_irregular = (int64_t) h[WTR_S_IRR]; cn.first_irregular = (int64_t) h[WTR_S_FIRST_IRR]; cn.n_unsorted = (int64_t) h[WTR_S_UNSORTED];
    cn.continues = (int64_t) h[WTR_S_CONTINUES];
    *counts = cn;
    if (cn.n_irregular) { *why = "irregular lines (counts: how many, and the first one's byte offset); the host sweep reads such text"; return 1; }
    if (cn.n_unsorted) { *why = "the BED records are not sorted"; return 1; }
    if (cn.n_runs >= (1ll << 31)) { *why = "2^31 records or more in one call"; return 1; }
    if (cn.n_runs > capacity || cn.n_seg > seg_capacity || cn.n_slow > slow_capacity) return 3;
    if (!l.run_read(WTR_K_WRITE, a.n_tiles, a) || !l.run_read(WTR_K_STATE, 1, a) || !l.to_host(state, a.st_out, sizeof(WtrState))) { *why = "write passes"; return 2; }
    return 0;
}

#endif  // WCV_NO_HOST

// The same rule on the host, without a device (a translation unit compiled with -DWT_EMU): one sweep over the lines with the
// parser above, every number through strtod (so n_slow counts, and nothing is left to patch: slow_rec / slow_off are still
// filled), text and outputs in host memory.  The same arguments, refusals, counts and return values as the door's.
#ifdef WT_EMU

static int wtr_host(const char *text, long long n_bytes, unsigned int flags, WtrState *state, int32_t *start, int32_t *finish, double *value,
                    long long capacity, int64_t *seg_off, int64_t *seg_name_off, int32_t *seg_name_len, long long seg_capacity, int64_t *slow_rec,
                    int64_t *slow_off, long long slow_capacity, WtrCounts *counts) {
    if (!state || !counts || n_bytes < 0 || capacity < 0 || seg_capacity < 0 || slow_capacity < 0 || (n_bytes > 0 && !text)) return 1;
    if (flags & ~(WTR_BED | WTR_EOF)) return 1;
    if (state->mode < WTR_M_BEDGRAPH || state->mode > WTR_M_VARIABLE || state->chrom_len < 0 || state->chrom_len > WTR_NAME_MAX || state->rec_len < 0 ||
        state->rec_len > WTR_NAME_MAX || n_bytes >= (1ll << 40)) return 1;
    WtrCounts cn = {};
    cn.first_irregular = -1;
    if (n_bytes == 0) { *counts = cn; return 0; }
    if (text[n_bytes - 1] != '\n' && !(flags & WTR_EOF)) return 1;
    WtrCtx c;
    c.text = (const unsigned char *) text; c.n = n_bytes; c.lo = 0; c.hi = 0; c.win = c.text; c.shift = 0;
    struct Rec { long long s, f, name_off, num_off; wtr_u64 bits; int name_len, slow, opens; };
    std::vector<Rec> recs;
    WtrState st = *state;
    std::string cur_chrom(st.chrom, (size_t) st.chrom_len), rec_name(st.rec_name, (size_t) st.rec_len);
    long long chrom_off = WTR_STATE_NAME;
    bool bed = (flags & WTR_BED) != 0;
    for (long long s = 0; s < n_bytes;) {
        long long e = s;
        while (e < n_bytes && text[e] != '\n') e++;             // (the whole line, however long)
        cn.n_lines++;
        const WtrLine ln = wtr_parse(c, s, e - s >= WTR_LINE_MAX ? s : e, flags);
        bool irregular = ln.kind == WTR_L_IRREGULAR;
        if (ln.kind == WTR_L_FIXED || ln.kind == WTR_L_VARIABLE) {
            const WtrHdr h = wtr_header(c, s, e, ln.kind == WTR_L_FIXED);
            st.mode = ln.kind == WTR_L_FIXED ? WTR_M_FIXED : WTR_M_VARIABLE;
            st.span = (int32_t) h.span; st.step = (int32_t) h.step; st.next = ln.kind == WTR_L_FIXED ? h.start : 0;
            cur_chrom.assign(text + h.chrom_off, (size_t) h.chrom_len);
            chrom_off = h.chrom_off;
        } else if (ln.kind == WTR_L_DATA) {
            Rec r = {ln.a + 1, ln.b + 1, s, ln.num_off, ln.vbits, ln.name_len, ln.slow, 0};
            std::string name;
            if (ln.nf == 4) {
                name.assign(text + s, (size_t) ln.name_len);
                if (!bed) { st.mode = WTR_M_BEDGRAPH; st.span = 0; st.step = 0; st.next = 0; cur_chrom.clear(); }
            } else {
                name = cur_chrom; r.name_off = chrom_off; r.name_len = (int) cur_chrom.size();
                if (ln.nf == 2) { irregular = st.mode != WTR_M_VARIABLE; r.s = ln.a; r.f = ln.a + st.span; }
                else { irregular = st.mode != WTR_M_FIXED; r.s = st.next; r.f = r.s + st.span; st.next += st.step; }
                if (r.s > (long long) INT32_MAX || r.f > (long long) INT32_MAX || r.s < (long long) INT32_MIN) irregular = true;
            }
            if (!irregular) {
                const bool have = !recs.empty() || st.rec_len > 0;
                r.opens = recs.empty() || name != rec_name;
                if (recs.empty()) cn.continues = have && name == rec_name;
                if (bed && have) {
                    const int d = strcmp(name.c_str(), rec_name.c_str());
                    if (d < 0 || (d == 0 && r.s < (long long) st.last_start)) cn.n_unsorted++;
                }
                if (r.slow) {
                    const std::string num(text + ln.num_off, (size_t) (e - ln.num_off));
                    const double v = wtr_strtod(num.c_str());
                    memcpy(&r.bits, &v, 8);
                }
                rec_name = name; st.last_start = (int32_t) r.s; st.rec_len = (int32_t) name.size();
                cn.n_seg += r.opens; cn.n_slow += r.slow;
            }
            recs.push_back(r);
        }
        if (irregular) {
            if (cn.n_irregular++ == 0) cn.first_irregular = s;
        }
        s = e + 1;
    }
    cn.n_runs = (int64_t) recs.size();
    *counts = cn;
    if (cn.n_irregular || cn.n_unsorted || cn.n_runs >= (1ll << 31)) return 1;
    if (cn.n_runs > capacity || cn.n_seg > seg_capacity || cn.n_slow > slow_capacity) return 3;
    long long g = 0, k = 0;
    for (size_t i = 0; i < recs.size(); i++) {
        const Rec &r = recs[i];
        start[i] = (int32_t) r.s; finish[i] = (int32_t) r.f;
        memcpy(&value[i], &r.bits, 8);
        if (r.opens) { seg_off[g] = (int64_t) i; seg_name_off[g] = r.name_off; seg_name_len[g] = r.name_len; g++; }
        if (r.slow) { slow_rec[k] = (int64_t) i; slow_off[k] = r.num_off; k++; }
    }
    if (!recs.empty()) seg_off[g] = cn.n_runs;
    st.chrom_len = (int32_t) cur_chrom.size();
    memset(st.chrom, 0, sizeof st.chrom); memcpy(st.chrom, cur_chrom.data(), cur_chrom.size());
    memset(st.rec_name, 0, sizeof st.rec_name); memcpy(st.rec_name, rec_name.data(), rec_name.size());
    if (bed) { st.mode = state->mode; }
    *state = st;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// ANY text, the reference's way (WtrRefReader): what serves a file once a line is irregular, WTAMD_NO_DEVICE_READ=1 and a build
// without the HIP units.  One line of at most 4999 bytes at a time, as fgets(5000) hands them over (wtr_ref_pieces cuts a
// longer line as fgets does); the fields by sscanf / strtok with their leniency -- a conversion that fails leaves the previous
// record's field in place --, the reference's messages and exit(1) for its "Badly formatted" and "Invalid header" cases and
// for an unsorted BED file.  On regular text it gives the records of the passes above (tests/test_read_emu.py).
// ---------------------------------------------------------------------------------------------------------------------
struct WtrRefReader {
    bool bed = false;
    int mode = WTR_M_BEDGRAPH, step = 0, span = 0;
    std::string chrom, filename;
    int start = 0, finish = 0;
    double value = 1;

    [[noreturn]] static void fail(const char *fmt, const char *arg) {
        fprintf(stderr, fmt, arg);
        exit(1);
    }
    // a header line (it is cut up in place)
    void header(char *line) {
        bool no_chrom = true, no_start = true, no_step = true;
        const char *seps = " \t=";
        char *tok = strtok(line, seps);
        span = 1;
        tok = strtok(NULL, seps);
        while (tok) {
            // (one test after the other, each on whatever token the one before left: the reference's chain of ifs)
            if (strcmp(tok, "chrom") == 0) {
                no_chrom = false;
                if (!(tok = strtok(NULL, seps))) fail("%s", "Empty wi->chromosome name!\n");
                chrom = tok;
            }
            if (strcmp(tok, "start") == 0) {
                no_start = false;
                if (!(tok = strtok(NULL, seps))) fail("%s", "Empty wi->start position!\n");
                sscanf(tok, "%i", &start);
            }
            if (strcmp(tok, "span") == 0) {
                if (!(tok = strtok(NULL, seps))) fail("%s", "Empty span length!\n");
                sscanf(tok, "%i", &span);
            }
            if (strcmp(tok, "step") == 0) {
                no_step = false;
                if (mode == WTR_M_VARIABLE) fail("%s", "Cannot specify step length on a variable length track\n");
                if (!(tok = strtok(NULL, seps))) fail("%s", "Empty step length!\n");
                sscanf(tok, "%i", &step);
            }
            tok = strtok(NULL, seps);
        }
        if ((mode == WTR_M_FIXED && (no_chrom || no_start || no_step)) || (mode == WTR_M_VARIABLE && no_chrom)) fail("Invalid header, missing data: %s\n", line);
        if (mode == WTR_M_FIXED) start = (int) ((unsigned int) start - (unsigned int) step);       // (the first data line adds it back)
    }
    // one line as fgets gave it (0-terminated, at most 4999 bytes): true when it is a record (chrom, start, finish, value)
    bool line(char *ln) {
        if (ln[0] == '#' || ln[0] == (char) EOF) return false;
        if (bed) {
            char name[5000];
            int a = start - 1, b = finish - 1;      // (the reference's locals are uninitialised; a line that fails keeps the record before)
            name[0] = 0;
            if (sscanf(ln, "%s\t%i\t%i", name, &a, &b) < 1) snprintf(name, sizeof name, "%s", chrom.c_str());
            a = (int) ((unsigned int) a + 1u); b = (int) ((unsigned int) b + 1u);
            const int d = strcmp(name, chrom.c_str());
            if (d < 0 || (d == 0 && a < start)) {
                fprintf(stderr, "Bed file %s is not sorted!\nPosition %s:%i is before %s:%i\n", filename.c_str(), name, a, chrom.c_str(), start);
                exit(1);
            }
            start = a; finish = b; chrom = name;
            return true;
        }
        if (strncmp("variableStep", ln, 12) == 0) { mode = WTR_M_VARIABLE; header(ln); return false; }
        if (strncmp("fixedStep", ln, 9) == 0) { mode = WTR_M_FIXED; header(ln); return false; }
        if (strncmp("track", ln, 5) == 0) return false;
        int words = ln[0] != ' ' && ln[0] != '\t' ? 1 : 0;
        for (const char *p = ln; *p; p++) if (*p == ' ' || *p == '\t') words++;
        if (words == 4) {
            char name[5000];
            name[0] = 0;
            mode = WTR_M_BEDGRAPH;
            sscanf(ln, "%s\t%i\t%i\t%lf", name, &start, &finish, &value);
            start = (int) ((unsigned int) start + 1u); finish = (int) ((unsigned int) finish + 1u);
            chrom = name;
        } else if (words == 2) {
            if (mode != WTR_M_VARIABLE) fail("Badly formatted fixed step line:\n%s", ln);
            sscanf(ln, "%i\t%lf", &start, &value);
            finish = (int) ((unsigned int) start + (unsigned int) span);
        } else if (words == 1) {
            if (mode != WTR_M_FIXED) fail("Badly formatted variable step line:\n%s", ln);
            sscanf(ln, "%lf", &value);
            start = (int) ((unsigned int) start + (unsigned int) step);
            finish = (int) ((unsigned int) start + (unsigned int) span);
        } else fail("Badly formatted wiggle or bed graph line :\n%s", ln);
        return true;
    }
    // after the chunks the device read: go on from their state (the last record's finish and value beside it)
    void resume(const WtrState &st, bool bed_, int last_finish, double last_value) {
        bed = bed_; mode = st.mode; step = st.step; span = st.span; finish = last_finish; value = last_value;
        const bool own = bed_ || st.mode == WTR_M_BEDGRAPH;
        chrom.assign(own ? st.rec_name : st.chrom, (size_t) (own ? st.rec_len : st.chrom_len));
        start = !bed_ && st.mode == WTR_M_FIXED ? (int) ((unsigned int) st.next - (unsigned int) st.step) : st.last_start;
    }
};

// the pieces fgets(line, 5000) cuts [p, e) into, one call of `f(char *piece)` each (a piece ends after a newline or at 4999 bytes)
template <class F>
static void wtr_ref_pieces(const char *p, const char *e, F f) {
    char buf[5000];
    while (p < e) {
        size_t n = 0;
        while (p + n < e && n < 4999) { n++; if (p[n - 1] == '\n') break; }
        memcpy(buf, p, n);
        buf[n] = 0;
        f(buf);
        p += n;
    }
}
#endif  // WT_EMU

#endif  // WT_READ_H_

