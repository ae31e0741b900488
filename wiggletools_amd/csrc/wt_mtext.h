// wt_mtext.h -- wig, bedGraph and paste text of a Multiplexer tile (device + -DWT_EMU): the reference's multi-column writer,
// printBlock of TeeMultiplexer / PasteMultiplexer (src/mWigWriter.c:56-133; the parser's `mwrite`, `mwrite_bg`, `apply_paste`),
// byte for byte.  This header is the single source of the logic.  It is compiled
//   * by hipcc for gfx950 inside csrc/wt_mtext.hip (the product),
//   * by g++ with -DWT_EMU inside tests/mtext_emu.cpp, which runs the workgroups of every pass one after the other in any order
//     on the CPU, and as the host sweep at the end (wtm_host; the drop-in layer compiles it too).
// "%lf", the digit writers, the last-setter mode scan and the state are those of wt_text.h.
//
// Input: the layout of wt_text.h (n_seg segments, seg_off, start / finish, a name per segment) and a tile, values[n * width],
// row r at values + r * width; optionally a prefix per entry (prefix bytes, prefix_off[n + 1]).
//
// THE RULE.  Entries are numbered from 0 across segments and printed in blocks of WTX_ENTRIES = 10000; every block starts out of
// point-by-point mode and without a previous entry.  L = finish - start.  ROW(r) is "\t%lf" of every cell of row r, then "\n".
// The mode is wt_text.h's (bedGraph whenever prefixes are given).  A point-by-point entry prints the "fixedStep" header under
// wt_text.h's conditions, then ROW(r) L times; any other entry prints "%s\t%i\t%i" (name, start - 1, finish - 1) and ROW(r); an
// entry with a prefix prints its prefix bytes and ROW(r).
//
//   cells   a workgroup owns max(1, WTM_CELLS / width) whole entries: a lane a cell, coalesced 8-byte loads; the cell's length
//           and its wide flag; the lengths of a row summed by integer adds in LDS (the order cannot matter) and stored, plus the
//           newline, into erow[entry]; the workgroup's wide count
//   mode    ONE WORKGROUP PER 10000-ENTRY BLOCK: validation and wt_text.h's last-setter scan, tiles of 256 entries; mode and
//           header flags into the upper bits of erow[entry]; every entry's byte count; the sum of every tile of 256 entries
//   scan    ONE workgroup: the tiles' sums into 64-bit bases in a fixed order; bytes, wide cells, bad entries
//   emit    a flat grid over the tiles of 256 entries.  The text of a tile is the text of its ITEMS in order -- a cell of a row,
//           once per copy of the row; the first item of an entry also carries the entry's head (header, name and coordinates, or
//           prefix), the last cell of a row its newline --: chunks of 256 items, a lane an item; the items' lengths scanned in LDS,
//           a carry from chunk to chunk; the chunk composed into wt_text.h's LDS window piece by piece (a byte of the window and
//           its address in `text` agree modulo 16), whole 16-byte lines stored as one store each, ragged ends byte by byte.  A
//           row or a prefix longer than the window simply spans chunks and pieces.  No workgroup reads `text` or writes a byte
//           that is not its own.  (A point-by-point row is formatted once per copy: its copies are items like any other, so
//           the same scan places them; composing it once and storing it L times would need a second alignment per copy.)
// No floating-point arithmetic and no global atomics anywhere; the same input gives the same bytes.
#ifndef WT_MTEXT_H_
#define WT_MTEXT_H_

#include "wt_text.h"

#define WTM_BLOCK WTX_BLOCK
#define WTM_MAX_WIDTH 65536                     // WTAMD_MTEXT_MAX_WIDTH
#define WTM_CELLS 2048                          // cells pass: cells of a workgroup (one entry where a row is longer)
#define WTM_STRICT 2u                           // WTAMD_MTEXT_STRICT (wtamd_trackset_mtext only)
#define WTM_ROW_MASK 0x00ffffffu                // erow: bytes of ROW (at most 65536 * 29 + 1)
#define WTM_PBP 0x01000000u                     // erow: the entry is point-by-point
#define WTM_HDR 0x02000000u                     // erow: ... and prints a header

enum { WTM_K_CELLS = 0, WTM_K_MODE, WTM_K_SCAN, WTM_K_EMIT, WTM_K_COUNT_ };

struct alignas(16) WtmLds {
    WtxLds x;                                   // the window (cells: the rows' sums), the masks, the carry, bad / wide per lane
    wtx_u64 sc[2][WTM_BLOCK];                   // lengths, scanned
    unsigned int voff[WTM_BLOCK + 1];           // emit: items before an entry of the tile
    wtx_u64 base;                               // emit: bytes of the tile before the chunk
};

struct WtmArgs {
    WtxArgs x;                                  // start, finish, n, seg_off, n_seg, names, name_off, flags (WTX_BEDGRAPH also where
                                                // prefixes are given), first, st_*, n_blocks, scalars, text, capacity
    const double *values;
    int width;
    const char *prefix;                         // may be NULL
    const int64_t *prefix_off;
    long long per_wg, n_cwg;                    // cells: entries of a workgroup, workgroups
    unsigned int *erow;                         // [n]
    unsigned int *cwide;                        // [n_cwg] wide cells of a cells workgroup
    wtx_u64 *tbytes;                            // [n_blocks * WTX_TILES] bytes of a tile; after the scan: bytes before it
    wtx_u64 *bad;                               // [n_blocks] bad entries of a block
};

// inclusive scan of sc[0] (complete, the workgroup in step), ending in sc[0]
WCV_DEV void wtm_scan(WtmLds *lds) {
    int cur = 0;
    for (int d = 1; d < WTM_BLOCK; d <<= 1) {
        WCV_LANES(l) { lds->sc[cur ^ 1][l] = lds->sc[cur][l] + (l >= d ? lds->sc[cur][l - d] : 0ull); }
        WCV_SYNC();
        cur ^= 1;
    }
}

// ---- cells ----
WCV_DEV void wtm_cells_block(const WtmArgs &a, long long b, WtmLds *lds) {
    int *rows = (int *) lds->x.win;
    const long long e0 = b * a.per_wg, e1 = e0 + a.per_wg < a.x.n ? e0 + a.per_wg : a.x.n;
    const int ne = (int) (e1 - e0);
    WCV_LANES(l) { for (int j = l; j < ne; j += WTM_BLOCK) rows[j] = 0; }
    WCV_SYNC();
    const long long c0 = e0 * a.width;
    const unsigned int nc = (unsigned int) ne * (unsigned int) a.width;        // (at most max(WTM_CELLS, WTM_MAX_WIDTH))
    WCV_LANES(l) {
        unsigned int wide = 0;
        int own = 0;
        for (unsigned int c = (unsigned int) l; c < nc; c += WTM_BLOCK) {
            const WtxNum num = wtx_num(a.values[c0 + c]);
            wide += num.kind == WTX_WIDE;
            const int len = 1 + (int) wtx_num_len(num);
            if (a.per_wg == 1) own += len; else wcv_add32(&rows[c / (unsigned int) a.width], len);
        }
        if (a.per_wg == 1 && own) wcv_add32(&rows[0], own);
        lds->x.wide[l] = wide;
    }
    WCV_SYNC();
    WCV_LANES(l) {
        for (int j = l; j < ne; j += WTM_BLOCK) a.erow[e0 + j] = (unsigned int) rows[j] + 1u;
        if (l == 0) {
            wtx_u64 wide = 0;
            for (int k = 0; k < WTM_BLOCK; k++) wide += lds->x.wide[k];
            a.cwide[b] = (unsigned int) (wide > 0xffffffffull ? 0xffffffffull : wide);
        }
    }
}

// ---- what an entry prints in front of its first row ----
WCV_DEV long long wtm_prefix_len(const WtmArgs &a, long long i) { return (long long) a.prefix_off[i + 1] - (long long) a.prefix_off[i]; }

WCV_DEV wtx_u64 wtm_head_len(const WtmArgs &a, long long i, int g, int32_t s, int32_t f, unsigned int w) {
    if (a.prefix) return (wtx_u64) wtm_prefix_len(a, i);
    const unsigned int nl = (unsigned int) (a.x.name_off[g + 1] - a.x.name_off[g]);
    if (w & WTM_PBP) return (w & WTM_HDR) ? 31u + nl + wtx_int_len(s) : 0u;
    return nl + 1u + wtx_int_len((long long) s - 1) + 1u + wtx_int_len((long long) f - 1);
}

// ---- mode ----
WCV_DEV void wtm_mode_block(const WtmArgs &a, long long block, WtmLds *lds) {
    const WtxArgs &x = a.x;
    const long long i0 = wtx_block_first(x, block), i1 = wtx_block_end(x, block);
    WCV_LANES(l) {
        lds->x.bad[l] = 0;
        if (l == 0) wtx_block_open(x, block, &lds->x);
    }
    WCV_SYNC();
    for (int t = 0; t < WTX_TILES; t++) {
        const long long e0 = i0 + (long long) t * WTM_BLOCK;
        WCV_LANES(l) { wtx_tile_mark(x, e0, i1, &lds->x, l); }
        WCV_SYNC();
        WCV_LANES(l) {
            const long long i = e0 + l;
            wtx_u64 bytes = 0;
            if (i < i1) {
                const int32_t s = x.start[i], f = x.finish[i];
                bool bad = s >= f || s == INT32_MIN;
                if (a.prefix && wtm_prefix_len(a, i) < 0) bad = true;
                const int g = (int) wcv_seg_of(x.seg_off, x.n_seg, i);
                unsigned int w = a.erow[i] & WTM_ROW_MASK;
                if (wtx_mode_at(&lds->x, l)) {
                    const int32_t before = x.finish[i > 0 ? i - 1 : 0];
                    const bool head = i == i0, first = head && !(block == 0 && x.st_prev);
                    const int pmode = head ? x.st_mode : wtx_mode_at(&lds->x, l - 1);
                    const int pfinish = head ? x.st_finish : before;
                    const int psame = head ? x.st_same : (int) (i - 1 >= (long long) x.seg_off[g]);
                    w |= WTM_PBP;
                    if (first || !pmode || !psame || s > pfinish) w |= WTM_HDR;
                }
                if (bad) lds->x.bad[l]++;
                else bytes = wtm_head_len(a, i, g, s, f, w) + (wtx_u64) (w & WTM_ROW_MASK) * (wtx_u64) ((w & WTM_PBP) ? f - s : 1);
                a.erow[i] = w;
            }
            lds->sc[0][l] = bytes;
        }
        WCV_SYNC();
        wtm_scan(lds);
        WCV_LANES(l) {
            if (l == 0) {
                a.tbytes[block * WTX_TILES + t] = lds->sc[0][WTM_BLOCK - 1];
                wtx_tile_close(&lds->x);
            }
        }
        WCV_SYNC();
    }
    WCV_LANES(l) {
        if (l == 0) {
            wtx_u64 bad = 0;
            for (int k = 0; k < WTM_BLOCK; k++) bad += lds->x.bad[k];
            a.bad[block] = bad;
            if (block == x.n_blocks - 1) {
                x.scalars[WTX_S_MODE] = (wtx_u64) lds->x.carry;
                x.scalars[WTX_S_FINISH] = (wtx_u64) (unsigned int) x.finish[x.n - 1];
            }
        }
    }
}

// ---- scan: one workgroup, a slice per lane, the 256 slice sums by lane 0 ----
WCV_DEV void wtm_scan_block(const WtmArgs &a, long long block, WtmLds *lds) {
    if (block != 0) return;
    const long long n_tiles = a.x.n_blocks * WTX_TILES;
    const long long per = (n_tiles + WTM_BLOCK - 1) / WTM_BLOCK, perb = (a.x.n_blocks + WTM_BLOCK - 1) / WTM_BLOCK, perc = (a.n_cwg + WTM_BLOCK - 1) / WTM_BLOCK;
    WCV_LANES(l) {
        wtx_u64 bytes = 0, bad = 0, wide = 0;
        for (long long t = (long long) l * per; t < (long long) (l + 1) * per && t < n_tiles; t++) bytes += a.tbytes[t];
        for (long long b = (long long) l * perb; b < (long long) (l + 1) * perb && b < a.x.n_blocks; b++) bad += a.bad[b];
        for (long long c = (long long) l * perc; c < (long long) (l + 1) * perc && c < a.n_cwg; c++) wide += a.cwide[c];
        lds->x.acc[l] = bytes; lds->sc[0][l] = bad; lds->sc[1][l] = wide;
    }
    WCV_SYNC();
    WCV_LANES(l) {
        if (l == 0) {
            wtx_u64 run = 0, bad = 0, wide = 0;
            for (int k = 0; k < WTM_BLOCK; k++) { const wtx_u64 c = lds->x.acc[k]; lds->x.acc[k] = run; run += c; bad += lds->sc[0][k]; wide += lds->sc[1][k]; }
            a.x.scalars[WTX_S_BYTES] = run; a.x.scalars[WTX_S_ERR] = bad; a.x.scalars[WTX_S_WIDE] = wide;
        }
    }
    WCV_SYNC();
    WCV_LANES(l) {
        wtx_u64 run = lds->x.acc[l];
        for (long long t = (long long) l * per; t < (long long) (l + 1) * per && t < n_tiles; t++) { const wtx_u64 c = a.tbytes[t]; a.tbytes[t] = run; run += c; }
    }
}

// ---- emit ----
struct WtmItem {
    long long i;                                // the entry
    int k, first;                               // the column; the entry's first item
    WtxNum num;
    wtx_u64 head, len;
};

// bytes [0, n) of src at text position p, as far as they lie in the window's piece
WCV_DEV long long wtm_put_bytes(const WtxOut &o, long long p, const char *src, long long n) {
    long long j0 = o.lo - p, j1 = o.hi - p;
    if (j0 < 0) j0 = 0;
    if (j1 > n) j1 = n;
    for (long long j = j0; j < j1; j++) o.win[o.shift + (p + j - o.lo)] = (unsigned char) src[j];
    return p + n;
}

// item r of entry j of the tile that starts at entry e0
WCV_DEV WtmItem wtm_item(const WtmArgs &a, long long e0, int j, unsigned int r) {
    WtmItem it;
    it.i = e0 + j;
    it.k = (int) (r % (unsigned int) a.width);
    it.first = r == 0;
    it.num = wtx_num(a.values[it.i * a.width + it.k]);
    it.head = 0;
    if (it.first) {
        const int g = a.prefix ? 0 : (int) wcv_seg_of(a.x.seg_off, a.x.n_seg, it.i);
        it.head = wtm_head_len(a, it.i, g, a.x.start[it.i], a.x.finish[it.i], a.erow[it.i]);
    }
    it.len = it.head + 1u + wtx_num_len(it.num) + (it.k == a.width - 1 ? 1u : 0u);
    return it;
}

WCV_DEV void wtm_compose(const WtmArgs &a, const WtmItem &it, const WtxOut &o, long long p) {
    if (it.first && it.head) {
        if (a.prefix) p = wtm_put_bytes(o, p, a.prefix + a.prefix_off[it.i], (long long) it.head);
        else {
            const int g = (int) wcv_seg_of(a.x.seg_off, a.x.n_seg, it.i);
            const char *name = a.x.names + a.x.name_off[g];
            const int nl = (int) (a.x.name_off[g + 1] - a.x.name_off[g]);
            const int32_t s = a.x.start[it.i], f = a.x.finish[it.i];
            if (a.erow[it.i] & WTM_PBP) {
                p = wtx_put_str(o, p, "fixedStep chrom=", 16);
                p = wtm_put_bytes(o, p, name, nl);
                p = wtx_put_str(o, p, " start=", 7);
                p = wtx_put_int(o, p, (long long) s);
                p = wtx_put_str(o, p, " step=1\n", 8);
            } else {
                p = wtm_put_bytes(o, p, name, nl);
                wtx_put(o, p++, '\t');
                p = wtx_put_int(o, p, (long long) s - 1);
                wtx_put(o, p++, '\t');
                p = wtx_put_int(o, p, (long long) f - 1);
            }
        }
    }
    wtx_put(o, p++, '\t');
    p = wtx_put_num(o, p, it.num);
    if (it.k == a.width - 1) wtx_put(o, p++, '\n');
}

WCV_DEV void wtm_emit_block(const WtmArgs &a, long long tile, WtmLds *lds) {
    const WtxArgs &x = a.x;
    const long long block = tile / WTX_TILES;
    const long long i1 = wtx_block_end(x, block), e0 = wtx_block_first(x, block) + (tile % WTX_TILES) * WTM_BLOCK;
    if (e0 >= i1) return;
    const wtx_u64 tile_at = a.tbytes[tile];                            // the tile's first byte in `text`
    WCV_LANES(l) {
        wtx_u64 items = 0;
        if (e0 + l < i1) {
            const unsigned int w = a.erow[e0 + l];
            items = (wtx_u64) a.width * (wtx_u64) ((w & WTM_PBP) ? x.finish[e0 + l] - x.start[e0 + l] : 1);
        }
        lds->sc[0][l] = items;
        if (l == 0) { lds->base = 0; lds->voff[0] = 0; }
    }
    WCV_SYNC();
    wtm_scan(lds);
    WCV_LANES(l) { lds->voff[l + 1] = (unsigned int) lds->sc[0][l]; }   // (at most 256 * 65536 * 5)
    WCV_SYNC();
    const unsigned int n_items = lds->voff[WTM_BLOCK];
    for (unsigned int q0 = 0; q0 < n_items; q0 += WTM_BLOCK) {
        WCV_LANES(l) {
            const unsigned int q = q0 + (unsigned int) l;
            wtx_u64 len = 0;
            if (q < n_items) {
                int lo = 0, hi = WTM_BLOCK;                             // voff[lo] <= q < voff[hi]
                while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (lds->voff[mid] <= q) lo = mid; else hi = mid; }
                lds->x.bad[l] = (unsigned int) lo;                      // (the lane's entry, kept for the pieces)
                len = wtm_item(a, e0, lo, q - lds->voff[lo]).len;
            }
            lds->sc[0][l] = len;
        }
        WCV_SYNC();
        wtm_scan(lds);
        const long long chunk_bytes = (long long) lds->sc[0][WTM_BLOCK - 1];
        const wtx_u64 chunk_at = tile_at + lds->base;
        for (long long p0 = 0; p0 < chunk_bytes; p0 += WTX_PIECE) {
            const long long len = chunk_bytes - p0 < WTX_PIECE ? chunk_bytes - p0 : WTX_PIECE;
            const unsigned long long addr = (unsigned long long) (uintptr_t) x.text + chunk_at + (wtx_u64) p0;
            const int shift = (int) (addr & 15ull);
            WCV_LANES(l) {
                const unsigned int q = q0 + (unsigned int) l;
                if (q < n_items) {
                    const long long end = (long long) lds->sc[0][l], beg = l ? (long long) lds->sc[0][l - 1] : 0;
                    if (beg < p0 + len && end > p0) {
                        const int j = (int) lds->x.bad[l];
                        const WtmItem it = wtm_item(a, e0, j, q - lds->voff[j]);
                        const WtxOut o = {lds->x.win, p0, p0 + len, shift};
                        wtm_compose(a, it, o, beg);
                    }
                }
            }
            WCV_SYNC();
            WCV_LANES(l) {
                char *dst = (char *) (uintptr_t) (addr - (unsigned long long) shift);          // 16-byte aligned; window byte j <-> dst[j]
                long long total = shift + len;
                const long long room = x.capacity - (long long) (chunk_at + (wtx_u64) p0) + shift;   // (never past the caller's buffer)
                if (total > room) total = room;
                for (long long c = l; c * 16 < total; c += WTM_BLOCK) {
                    const long long lo = c * 16, hi = lo + 16;
                    if (lo >= shift && hi <= total) *(WtxV4 *) (dst + lo) = *(const WtxV4 *) (lds->x.win + lo);
                    else for (long long j = lo < shift ? shift : lo; j < (hi < total ? hi : total); j++) dst[j] = (char) lds->x.win[j];
                }
            }
            WCV_SYNC();
        }
        WCV_LANES(l) { if (l == 0) lds->base += (wtx_u64) chunk_bytes; }
        WCV_SYNC();
    }
}

WCV_DEV void wtm_run_block(int kernel, const WtmArgs &a, long long block, WtmLds *lds) {
    switch (kernel) {
    case WTM_K_CELLS: wtm_cells_block(a, block, lds); break;
    case WTM_K_MODE: wtm_mode_block(a, block, lds); break;
    case WTM_K_SCAN: wtm_scan_block(a, block, lds); break;
    case WTM_K_EMIT: wtm_emit_block(a, block, lds); break;
    default: break;
    }
}

// what every entry checks before it touches anything; "" when fine
static inline const char *wtm_check(long long n_seg, const int64_t *seg_off, const char *const *seg_name, const int32_t *start, const int32_t *finish,
                                    const double *values, int width, const char *prefix, const int64_t *prefix_off, unsigned int flags,
                                    const WtxState *state, const void *text, long long capacity, const int64_t *n_bytes, const int64_t *n_wide) {
    if (width < 1 || width > WTM_MAX_WIDTH) return "width outside 1 .. WTAMD_MTEXT_MAX_WIDTH";
    if ((prefix != nullptr) != (prefix_off != nullptr)) return "prefix and prefix_off go together";
    return wtx_check(n_seg, seg_off, seg_name, start, finish, values, flags, state, text, capacity, n_bytes, n_wide);
}

// ---------------------------------------------------------------------------------------------------------------------
// The door, written once over a Launcher: the one of wt_cover.h (alloc, release, zero, to_host, to_device) with
//     bool run_mtext(int kernel, long long blocks, const WtmArgs &a)     and     bool sync()
// Return value: 0 fine, 1 bad argument, 2 launcher failure, 3 capacity (*n_bytes: the size needed).  Nothing is written to text
// or state unless the value is 0.  Temporary memory: 4 bytes per entry; 8 bytes per tile of 256 entries (40 tiles per 10000
// entries, the first and the last block's included); 8 bytes per 10000 entries; 4 bytes per max(1, 2048 / width) entries; 12
// bytes and its name per segment; 64 of scalars.
// ---------------------------------------------------------------------------------------------------------------------
#ifndef WCV_NO_HOST

template <class L>
static int wtm_door(L &l, long long n_seg, const int64_t *seg_off, const char *const *seg_name, const int32_t *start, const int32_t *finish,
                    const double *values, int width, const char *prefix, const int64_t *prefix_off, unsigned int flags, WtxState *state, char *text,
                    long long capacity, int64_t *n_bytes, int64_t *n_wide, const char **why) {
    *why = wtm_check(n_seg, seg_off, seg_name, start, finish, values, width, prefix, prefix_off, flags, state, text, capacity, n_bytes, n_wide);
    if (**why) return 1;
    WtmArgs a = {};
    WtxArgs &x = a.x;
    x.start = start; x.finish = finish;
    x.n = n_seg ? (long long) seg_off[n_seg] : 0;
    *n_wide = 0;
    if (x.n == 0) { *n_bytes = 0; return 0; }
    x.n_seg = n_seg; x.flags = prefix ? flags | WTX_BEDGRAPH : flags; x.text = text; x.capacity = capacity;
    a.values = values; a.width = width; a.prefix = prefix; a.prefix_off = prefix_off;
    const int in_block = state ? (int) state->in_block : 0;
    x.first = WTX_ENTRIES - in_block;
    x.st_prev = in_block > 0;
    if (x.st_prev) { x.st_mode = state->point_by_point != 0; x.st_finish = state->last_finish; x.st_same = state->continues != 0; }
    x.n_blocks = x.n <= x.first ? 1 : 1 + wcv_blocks(x.n - x.first, WTX_ENTRIES);
    a.per_wg = width >= WTM_CELLS ? 1 : WTM_CELLS / width;
    a.n_cwg = wcv_blocks(x.n, a.per_wg);
    std::string names;
    std::vector<int32_t> name_off((size_t) n_seg + 1, 0);
    for (long long g = 0; g < n_seg; g++) { names += seg_name[g]; name_off[(size_t) g + 1] = (int32_t) names.size(); }
    WcvScope<L> sc(l);
    int64_t *d_seg = nullptr;
    char *d_names = nullptr;
    int32_t *d_noff = nullptr;
    if (!sc.get(&d_seg, (size_t) n_seg + 1) || !sc.get(&d_names, names.size()) || !sc.get(&d_noff, (size_t) n_seg + 1) ||
        !sc.get(&a.erow, (size_t) x.n) || !sc.get(&a.cwide, (size_t) a.n_cwg) || !sc.get(&a.tbytes, (size_t) (x.n_blocks * WTX_TILES)) ||
        !sc.get(&a.bad, (size_t) x.n_blocks) || !sc.get(&x.scalars, (size_t) WTX_S_N))
        { *why = "device memory"; return 2; }
    x.seg_off = d_seg; x.names = d_names; x.name_off = d_noff;
    wtx_u64 h_sc[WTX_S_N] = {};
    if (!l.to_device(d_seg, seg_off, sizeof(int64_t) * ((size_t) n_seg + 1)) || !l.to_device(d_names, names.data(), names.size()) ||
        !l.to_device(d_noff, name_off.data(), sizeof(int32_t) * ((size_t) n_seg + 1)) || !l.zero(x.scalars, sizeof h_sc))
        { *why = "copy"; return 2; }
    if (!l.run_mtext(WTM_K_CELLS, a.n_cwg, a) || !l.run_mtext(WTM_K_MODE, x.n_blocks, a) || !l.run_mtext(WTM_K_SCAN, 1, a) ||
        !l.to_host(h_sc, x.scalars, sizeof h_sc))
        { *why = "measuring passes"; return 2; }
    if (h_sc[WTX_S_ERR]) { *why = "an entry with start >= finish or start == INT32_MIN, or prefix offsets that decrease"; return 1; }
    if (h_sc[WTX_S_WIDE]) { *n_wide = (int64_t) h_sc[WTX_S_WIDE]; *why = "a finite value of 2^64 or more (use the host sweep)"; return 1; }
    if (h_sc[WTX_S_BYTES] > (wtx_u64) capacity) { *n_bytes = (int64_t) h_sc[WTX_S_BYTES]; return 3; }
    if (!l.run_mtext(WTM_K_EMIT, x.n_blocks * WTX_TILES, a) || !l.sync()) { *why = "emit pass"; return 2; }
    *n_bytes = (int64_t) h_sc[WTX_S_BYTES];
    if (state) {
        state->in_block = (int32_t) ((in_block + x.n) % WTX_ENTRIES);
        state->point_by_point = (int32_t) h_sc[WTX_S_MODE];
        state->last_finish = (int32_t) (unsigned int) h_sc[WTX_S_FINISH];
        state->continues = 1;
    }
    return 0;
}

#endif  // WCV_NO_HOST

// The same rule on the host, without a device (a translation unit compiled with -DWT_EMU): one sweep, values through
// snprintf("%f"), so that a wide value is printed too (*n_wide counts them; they are no refusal here).  Otherwise the same
// arguments, refusals and return values as the door's, everything in host memory; the same bytes.
#ifdef WT_EMU

static int wtm_host(long long n_seg, const int64_t *seg_off, const char *const *seg_name, const int32_t *start, const int32_t *finish,
                    const double *values, int width, const char *prefix, const int64_t *prefix_off, unsigned int flags, WtxState *state, char *text,
                    long long capacity, int64_t *n_bytes, int64_t *n_wide) {
    if (*wtm_check(n_seg, seg_off, seg_name, start, finish, values, width, prefix, prefix_off, flags, state, text, capacity, n_bytes, n_wide)) return 1;
    const long long n = n_seg ? (long long) seg_off[n_seg] : 0;
    *n_wide = 0;
    if (n == 0) { *n_bytes = 0; return 0; }
    for (long long i = 0; i < n; i++) if (start[i] >= finish[i] || start[i] == INT32_MIN || (prefix && prefix_off[i + 1] < prefix_off[i])) return 1;
    WtxState st = {0, 0, 0, 0};
    if (state && state->in_block > 0) st = *state;
    const bool bed = (flags & WTX_BEDGRAPH) != 0 || prefix != nullptr;
    std::string out, row;
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
            row.clear();
            for (int k = 0; k < width; k++) {
                const double v = values[i * width + k];
                if (v - v == 0.0 && fabs(v) >= 18446744073709551616.0) wide++;
                row.append(buf, (size_t) snprintf(buf, sizeof buf, "\t%f", v));
            }
            row += '\n';
            if (mode) {
                if (!have_prev || !pmode || !same || start[i] > st.last_finish) {
                    out += "fixedStep chrom="; out += seg_name[g]; out += " start="; out += std::to_string(start[i]); out += " step=1\n";
                }
                for (long long j = 0; j < L; j++) out += row;
            } else {
                if (prefix) out.append(prefix + prefix_off[i], (size_t) (prefix_off[i + 1] - prefix_off[i]));
                else { out += seg_name[g]; out += '\t'; out += std::to_string((long long) start[i] - 1); out += '\t'; out += std::to_string((long long) finish[i] - 1); }
                out += row;
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

#endif  // WT_MTEXT_H_
