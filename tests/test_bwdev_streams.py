"""BigWig sections through the bulk door of the pipe (wtamd_pipe_bw_reserve / wtamd_pipe_submit_bw): the device decoder
(csrc/wt_inflate.h, csrc/wt_bwdev_core.h, csrc/wt_bwdev.hip) against a plain reference -- zlib.decompress, the section
layout of the published format (tests/bw_indep_reader.py parse_section) and the reference reader's conventions restated
in numpy (1-based starts, 10 000-bp stretches, the clip window, the chrom-id filter, range_lo / range_hi).

A one-track pipe with op `sum` emits exactly the decoded pieces: coordinates must match and values bit for bit.  Several
tracks go through `mean` against the oracle.  Every accepted batch reports bw_error() == 0 -- a batch the device rejects
is never quietly decoded elsewhere here.

"emu": the kernels' per-lane / per-item code compiled for the host (tests/emu/wt_pipe_emu.cpp); "amd" (-m gpu): the
product's pipe.  Only streams that inflate cleanly travel to the device; corrupted streams stay in the CPU tests."""
import ctypes as C
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from bw_indep_reader import parse_section
from test_bwdev import _streams
from test_pipe import _lib_for
from wiggletools_amd.pipe import BwTrack, Pipe
from wiggletools_amd.runlists import RunLists

STRETCH = 10000
INT32_MAX = 2 ** 31 - 1
MAX_COORD = INT32_MAX - 65536              # WTAMD_MAX_COORD
# bytes of which every 4-byte word is a finite, normal float32 (top byte 0x38..0x47 or 0xB8..0xC7: |v| in 2^-15 .. 2^17)
FBYTES = np.array(list(range(0x38, 0x48)) + list(range(0xB8, 0xC8)), np.uint8)
STRATEGIES = (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED)
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(params=["emu", pytest.param("amd", marks=pytest.mark.gpu)])
def lib(request):
    return _lib_for(request.param)


def _backend(lib):
    return "emu" if lib is not None else "amd"


# ---------------------------------------------------------------------------------------------------------------------
# the reference: pieces of a section's items as the reader hands them on (src/bigWiggleReader.c:36-83,125-145)

def ref_pieces(s0, e0, v, chrom_len, box, clip_lo, clip_hi):
    """Items 0-based half-open -> pieces (start 1-based, finish exclusive, value): cut at the 10 000-bp stretch edges
    1 + 10000 k (stretches that start at or beyond the chromosome's length are never visited) when `box`, clipped to
    [clip_lo, clip_hi) and dropped when empty; in item order."""
    s = np.asarray(s0, np.int64) + 1
    f = np.asarray(e0, np.int64) + 1
    v = np.asarray(v, np.float32)
    lo, hi = int(clip_lo), int(clip_hi)
    if not box:
        a, b = np.maximum(s, lo), np.minimum(f, hi)
        m = a < b
        return a[m], b[m], v[m]
    keep = (f > lo) & (s < hi)
    s, f, v = s[keep], f[keep], v[keep]
    k0 = (np.maximum(s, lo) - 1) // STRETCH
    lim = np.minimum(np.minimum(f, hi), int(chrom_len))
    k1 = (lim - 2) // STRETCH                # last k with 1 + 10000 k < lim
    n = np.maximum(k1 - k0 + 1, 0)
    idx = np.repeat(np.arange(len(s)), n)
    first = np.cumsum(n) - n
    k = k0[idx] + (np.arange(len(idx)) - first[idx])
    a = 1 + STRETCH * k
    ps = np.maximum(np.maximum(s[idx], a), lo)
    pf = np.minimum(np.minimum(f[idx], a + STRETCH), hi)
    m = ps < pf
    return ps[m], pf[m], v[idx][m]


def test_reference_boxing_matches_reader_rule():
    """The restatement above on the literal cases of tests/test_bigwig.py::test_boxing_matches_reference_reader_rule."""
    def run(items, length, box):
        s, f, v = ref_pieces([a for a, _, _ in items], [b for _, b, _ in items], [x for _, _, x in items], length, box, -INT32_MAX, INT32_MAX)
        return list(zip(s.tolist(), f.tolist(), v.tolist()))
    chr_a = [(5, 9995, 1.0), (9995, 10005, 2.0), (19990, 30001, 3.0)]
    assert run(chr_a, 30001, True) == [(6, 9996, 1.0), (9996, 10001, 2.0), (10001, 10006, 2.0), (19991, 20001, 3.0), (20001, 30001, 3.0)]
    assert [p[:2] for p in run([(0, 25000, 7.0)], 25000, True)] == [(1, 10001), (10001, 20001), (20001, 25001)]
    assert [p[:2] for p in run(chr_a, 30001, False)] == [(6, 9996), (9996, 10006), (19991, 30002)]
    # the clip window cuts pieces and starts the stretch walk where it begins
    s, f, _ = ref_pieces([0], [25000], [1.0], 25000, True, 15000, 20500)
    assert list(zip(s.tolist(), f.tolist())) == [(15000, 20001), (20001, 20500)]


# ---------------------------------------------------------------------------------------------------------------------
# sections and streams

def section_bytes(cid, typ, s0, e0, vbits, count=None):
    """Plain bytes of a section of type 1 (bedGraph), 2 (variableStep) or 3 (fixedStep); vbits: uint32 value bits."""
    s0, e0, vbits = (np.asarray(x, np.uint32) for x in (s0, e0, vbits))
    n = len(vbits)
    span = int(e0[0] - s0[0]) if n else 1
    step = int(s0[1] - s0[0]) if n > 1 else span
    if typ == 1:
        body = np.stack([s0, e0, vbits], 1).astype("<u4").tobytes()
        step = span = 0
    elif typ == 2:
        body = np.stack([s0, vbits], 1).astype("<u4").tobytes()
        step = 0
    else:
        body = vbits.astype("<u4").tobytes()
    c_start, c_end = (int(s0[0]), int(e0[-1])) if n else (0, 0)
    return struct.pack("<IIIIIBBH", cid, c_start, c_end, step, span, typ, 0, n if count is None else count) + body


def items(rng, typ, pos, n, vbits=None):
    """n items of a section of type `typ` from 0-based position pos: (s0, e0, vbits, next free position)."""
    if vbits is None:
        vbits = (rng.integers(0, 800, n) / 8).astype(np.float32).view(np.uint32)
    if typ == 1:
        ln = rng.integers(1, 40, n)
        gap = (rng.random(n) < 0.1) * rng.integers(1, 300, n)
        e = pos + np.cumsum(ln + gap)
        s = e - ln
    else:
        span = int(rng.integers(1, 30))
        step = span + (int(rng.integers(0, 20)) if typ == 3 else 0)
        if typ == 3:
            s = pos + step * np.arange(n)
        else:
            s = pos + np.cumsum(span + rng.integers(0, 25, n)) - span
        e = s + span
    return s.astype(np.int64), e.astype(np.int64), np.asarray(vbits, np.uint32), int(e[-1]) + int(rng.integers(0, 5000))


def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem=8, flush=None):
    """A zlib stream of raw; flush: Z_SYNC_FLUSH / Z_FULL_FLUSH at a third and two thirds (empty stored blocks)."""
    co = zlib.compressobj(level, zlib.DEFLATED, 15, mem, strategy)
    if flush is None or len(raw) < 3:
        return co.compress(raw) + co.flush()
    a, b = len(raw) // 3, 2 * len(raw) // 3
    return co.compress(raw[:a]) + co.flush(flush) + co.compress(raw[a:b]) + co.flush(flush) + co.compress(raw[b:]) + co.flush()


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):             # LSB first
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, value, nbits):            # Huffman codes: MSB first
        self.put(int("{:0{}b}".format(value, nbits)[::-1], 2), nbits)

    def done(self):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
          8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def fixed_huffman_zlib(symbols):
    """A zlib stream of ONE fixed-Huffman block (RFC 1951 3.2.6) from symbols: ints (literals) or (length, distance)
    -- matches zlib's own deflate never emits, e.g. at distance 32 768.  Returns (stream, plain bytes)."""
    w = _Bits()
    w.put(1, 1)
    w.put(1, 2)
    plain = bytearray()

    def litlen(sym):
        if sym < 144:
            w.code(0x30 + sym, 8)
        elif sym < 256:
            w.code(0x190 + sym - 144, 9)
        elif sym < 280:
            w.code(sym - 256, 7)
        else:
            w.code(0xC0 + sym - 280, 8)
    for sym in symbols:
        if isinstance(sym, tuple):
            ln, d = sym
            assert 3 <= ln <= 258 and 1 <= d <= min(32768, len(plain))
            c = max(i for i in range(29) if _LBASE[i] <= ln) if ln < 258 else 28
            litlen(257 + c)
            w.put(ln - _LBASE[c], _LEXT[c])
            dc = max(i for i in range(30) if _DBASE[i] <= d)
            w.code(dc, 5)
            w.put(d - _DBASE[dc], _DEXT[dc])
            for _ in range(ln):
                plain.append(plain[-d])
        else:
            litlen(sym)
            plain.append(sym)
    litlen(256)
    body = w.done()
    stream = b"\x78\x01" + body + struct.pack(">I", zlib.adler32(bytes(plain)))
    assert zlib.decompress(stream) == bytes(plain)
    return stream, bytes(plain)


class Sec:
    """One section of a batch: its plain bytes, the bytes that travel (zlib stream or the plain bytes) and its index
    leaf's extents (0-based half-open)."""

    def __init__(self, plain, comp, leaf=None):
        self.plain, self.comp = plain, comp
        if leaf is None:
            cid, s, e, v = parse_section(plain)
            leaf = (int(s.min()), int(e.max())) if len(s) else (0, 0)
        self.leaf = leaf


def mk(rng, cid, typ, pos, n, compress=True, vbits=None, **z):
    s, e, vb, nxt = items(rng, typ, pos, n, vbits)
    plain = section_bytes(cid, typ, s, e, vb)
    return Sec(plain, deflate(plain, **z) if compress else plain), nxt


class Track:
    def __init__(self, secs, compressed=True, chrom_id=0, chrom_len=INT32_MAX - 1, box=True, clip=(-INT32_MAX, INT32_MAX), plain_bytes=None):
        self.secs, self.compressed, self.chrom_id, self.chrom_len, self.box, self.clip = secs, compressed, chrom_id, chrom_len, box, clip
        self.plain_bytes = plain_bytes if plain_bytes is not None else max([len(x.plain) for x in secs] + [24])

    def pieces(self):
        """The reference: what the reader makes of this track's sections."""
        S, F, V = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.float32)]
        for x in self.secs:
            plain = zlib.decompress(x.comp) if self.compressed else x.comp
            assert plain == x.plain
            cid, s0, e0, v = parse_section(plain)
            if cid != self.chrom_id:
                continue
            s, f, v = ref_pieces(s0, e0, v, self.chrom_len, self.box, *self.clip)
            S.append(s); F.append(f); V.append(v)
        return np.concatenate(S), np.concatenate(F), np.concatenate(V)


def submit(pipe, tracks, lo=-INT32_MAX, hi=INT32_MAX, rng=None):
    """acquire -> bw_reserve -> file bytes + tables -> submit_bw.  Sections sit at odd offsets (any alignment)."""
    rng = rng or np.random.default_rng(0)
    pipe.acquire()
    secs = [(t, x) for t, tk in enumerate(tracks) for x in tk.secs]
    gaps = rng.integers(0, 16, len(secs) + 1)
    n_bytes = int(sum(len(x.comp) for _, x in secs) + gaps.sum())
    data, table = pipe.bw_reserve(n_bytes, len(secs))
    at = int(gaps[0])
    for q, (t, x) in enumerate(secs):
        data[at:at + len(x.comp)] = np.frombuffer(x.comp, np.uint8)
        table[q].comp_off, table[q].comp_size, table[q].track = at, len(x.comp), t
        table[q].leaf_start, table[q].leaf_end = x.leaf
        at += len(x.comp) + int(gaps[q + 1])
    tk, first = [], 0
    for tr in tracks:
        lo_c, hi_c = tr.clip
        tk.append(BwTrack(tr.chrom_id, tr.chrom_len, int(tr.box), int(tr.compressed), lo_c, hi_c, first, len(tr.secs), tr.plain_bytes, 0))
        first += len(tr.secs)
    pipe.submit_bw(n_bytes, len(secs), tk, lo, hi)
    return len(secs)


def collect_ok(pipe):
    s, f, v = pipe.collect(copy=True)
    pipe.release()
    assert pipe.bw_error() == 0
    return s, f, v


def sum_pipe(lib, depth=1):
    return Pipe(1, "sum", n_slots=depth + 1, lib=lib, max_runs=1 << 23, max_intervals=1 << 16)


def check_one_track(got, track, lo=-INT32_MAX, hi=INT32_MAX, what=""):
    """1-track sum == the pieces with start in [lo, hi): coordinates exactly, values bit for bit."""
    s, f, v = track.pieces()
    m = (s >= lo) & (s < hi)
    s, f, v = s[m], f[m], v[m]
    gs, gf, gv = got
    assert len(gs) == len(s), (what, len(gs), len(s))
    bad = np.flatnonzero((gs != s) | (gf != f))
    assert not len(bad), (what, int(bad[0]), gs[bad[0]], gf[bad[0]], s[bad[0]], f[bad[0]])
    g32 = gv.astype(np.float32)
    assert np.array_equal(g32.astype(np.float64), gv), what            # float32-exact values
    bad = np.flatnonzero(g32.view(np.uint32) != v.view(np.uint32))
    assert not len(bad), (what, int(bad[0]), float(gv[bad[0]]), float(v[bad[0]]))
    return len(s)


def run_one_track(lib, track, lo=-INT32_MAX, hi=INT32_MAX, what=""):
    p = sum_pipe(lib)
    submit(p, [track], lo, hi)
    got = collect_ok(p)
    p.close()
    return check_one_track(got, track, lo, hi, what)


def check_mean(lib, oracle, tracks, what=""):
    """n tracks, op mean == the oracle over the reference's pieces."""
    p = Pipe(len(tracks), "mean", n_slots=2, lib=lib, max_runs=1 << 23)
    submit(p, tracks)
    gs, gf, gv = collect_ok(p)
    p.close()
    seg, S, F, V = [0], [], [], []
    for t in tracks:
        s, f, v = t.pieces()
        S.append(s); F.append(f); V.append(v)
        seg.append(seg[-1] + len(s))
    rl = RunLists(1, len(tracks), seg, np.concatenate(S), np.concatenate(F), np.concatenate(V).astype(np.float32))
    c, s, f, v = oracle.reduce(rl.as_dict(), "mean")
    assert len(gs) == len(s), (what, len(gs), len(s))
    assert np.array_equal(gs, s) and np.array_equal(gf, f), what
    assert np.array_equal(gv, v), what
    return len(s)


# ---------------------------------------------------------------------------------------------------------------------
# a. the zlib matrix

def _matrix_sections(rng, cid=0):
    secs, pos, k = [], 1000, 0
    for level in range(10):
        for strategy in STRATEGIES:
            for mem in (1, 8, 9):
                typ = 1 + k % 3
                n = int(rng.integers(1, 1500)) if k % 7 else 1
                flush = (None, zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH)[k % 3]
                x, pos = mk(rng, cid, typ, pos, n, level=level, strategy=strategy, mem=mem, flush=flush)
                secs.append(x)
                k += 1
    # the item limit of a section, every type; stored ones (level 0: > 64 KiB plain, several stored blocks)
    for typ in (1, 2, 3):
        for level in (0, 1, 9):
            x, pos = mk(rng, cid, typ, pos, 65535, level=level)
            secs.append(x)
    return secs


def test_zlib_matrix(lib, oracle):
    """Levels 0-9 x the five strategies x memLevels 1 / 8 / 9, one block and several (SYNC / FULL flushes), section
    types 1 / 2 / 3 from 1 to 65 535 items -- compressed and uncompressed (compressed = 0), boxed and not."""
    rng = np.random.default_rng(7)
    secs = _matrix_sections(rng)
    assert any(len(x.plain) > 65536 and len(x.comp) > len(x.plain) for x in secs)       # stored: several stored blocks
    n = run_one_track(lib, Track(secs), what="matrix box")
    n += run_one_track(lib, Track(secs, box=False), what="matrix unboxed")
    raw = [Sec(x.plain, x.plain, x.leaf) for x in secs]
    n += run_one_track(lib, Track(raw, compressed=False), what="matrix raw")
    assert n > 3 * 200000
    print("zlib matrix: %d sections x 3, %d pieces" % (len(secs), n))


def test_streams_of_the_lane_tests_as_sections(lib):
    """The streams of tests/test_bwdev.py _streams() (the host build's matrix) on the device: their bytes as the values
    of fixedStep sections -- zlib-wrapped streams only (sections always are), byte streams padded to whole words of
    finite values."""
    rng = np.random.default_rng(3)
    secs, pos = [], 0
    for trial, raw, comp, is_raw in _streams():
        if is_raw or len(raw) < 4:
            continue
        body = np.frombuffer(raw[:len(raw) // 4 * 4], np.uint8).copy()
        body[3::4] = FBYTES[body[3::4] % 32]          # finite floats: the top byte of every word from FBYTES
        n = min(len(body) // 4, 65535)
        x, pos = mk(rng, 0, 3, pos, n, vbits=body[:4 * n].view("<u4"), level=trial % 10, strategy=STRATEGIES[trial % 5],
                    flush=(None, zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH)[trial % 3])
        secs.append(x)
    n = run_one_track(lib, Track(secs), what="streams")
    print("lane-test streams: %d sections, %d pieces" % (len(secs), n))


# ---------------------------------------------------------------------------------------------------------------------
# b. match geometry

def _period_sections(rng, periods, levels=(1, 6, 9), n_bytes=2048):
    secs, pos = [], 0
    for p in periods:
        unit = FBYTES[rng.integers(0, 32, p)]
        body = np.resize(unit, n_bytes)
        for level in levels:
            s, e, vb, pos = items(rng, 3, pos, n_bytes // 4, body.view("<u4"))
            plain = section_bytes(0, 3, s, e, vb)
            secs.append(Sec(plain, deflate(plain, level=level)))
    return secs


def _match_sections(rng):
    """Hand-made fixed-Huffman streams: every match length 3..258 at distances on both sides of the ring's limit and
    at 32 768, behind 0..3 literals (every output alignment)."""
    secs, pos = [], 0
    for d in (1, 2, 3, 4, 5, 7, 8, 15, 16, 27, 28, 29, 31, 32, 33, 36, 60, 64, 65, 100, 252, 256, 257, 1000, 32768):
        prefix = FBYTES[rng.integers(0, 32, max(d, 64))].tolist()
        syms = list(prefix)
        for ln in range(3, 259):
            syms.append((ln, d))
            syms += FBYTES[rng.integers(0, 32, int(rng.integers(0, 4)))].tolist()
        out = sum(1 if not isinstance(q, tuple) else q[0] for q in syms)
        syms += FBYTES[rng.integers(0, 32, (-out) % 4)].tolist()
        out = sum(1 if not isinstance(q, tuple) else q[0] for q in syms)
        n = out // 4
        span = int(rng.integers(1, 4))
        head = struct.pack("<IIIIIBBH", 0, pos, pos + n * span, span, span, 3, 0, n)
        comp, plain = fixed_huffman_zlib(list(head) + syms)
        secs.append(Sec(plain, comp))
        pos += n * span + 7
    return secs


def test_match_geometry(lib):
    """Periods 1..72 and 248..260 (zlib levels 1 / 6 / 9: matches just inside and beyond the LDS ring, far copies of
    output stored one or two steps earlier) and exact (length, distance) pairs, lengths 3..258 at every alignment,
    distance 32 768 included."""
    rng = np.random.default_rng(11)
    per = _period_sections(rng, list(range(1, 73)) + list(range(248, 261)))
    n = run_one_track(lib, Track(per), what="periods")
    ms = _match_sections(rng)
    n += run_one_track(lib, Track(ms, box=False), what="matches")
    print("match geometry: %d period sections, %d match sections, %d pieces" % (len(per), len(ms), n))


# ---------------------------------------------------------------------------------------------------------------------
# c. wavefront mix, d. batch shapes

def _fib_literals(rng):
    """Literal-only data whose dynamic Huffman code needs 15-bit codes (Fibonacci frequencies)."""
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    sym = np.repeat(FBYTES[:22], fib)
    return sym[rng.permutation(len(sym))][:4 * (len(sym) // 4)]


def _mixed_tracks(rng, n_tracks=9):
    """Tracks of mixed sections so that every 64-lane wavefront holds stored, fixed, dynamic, long-code and raw lanes,
    1-item sections next to 65 535-item ones; one track without sections, one with a section of another chromosome,
    different plain_bytes, clip windows that cut items."""
    long_codes = _fib_literals(rng)
    tracks = []
    for t in range(n_tracks):
        comp = t % 3 != 2
        secs, pos = [], int(rng.integers(0, 100))
        if t == 4:
            tracks.append(Track([], compressed=comp))
            continue
        for q in range(22):
            if t == 6 and q == 4:       # a section of another chromosome between two of this one: yields nothing
                x, pos = mk(rng, 1, 1, pos, 30, comp)
                secs.append(x)
            kind = (q + t) % 6
            if kind == 0:
                x, pos = mk(rng, 0, 1 + q % 3, pos, int(rng.integers(50, 400)), comp, level=0)
            elif kind == 1:
                x, pos = mk(rng, 0, 1 + q % 3, pos, int(rng.integers(50, 400)), comp, strategy=zlib.Z_FIXED)
            elif kind == 2:
                x, pos = mk(rng, 0, 1 + q % 3, pos, int(rng.integers(50, 3000)), comp, level=6)
            elif kind == 3:
                x, pos = mk(rng, 0, 3, pos, len(long_codes) // 4, comp, vbits=long_codes.view("<u4"), strategy=zlib.Z_HUFFMAN_ONLY)
            elif kind == 4:
                x, pos = mk(rng, 0, 1 + q % 3, pos, 1, comp)
            else:
                x, pos = mk(rng, 0, 3, pos, 65535 if q == 5 and t < 3 else int(rng.integers(1, 40)), comp, level=1)
            secs.append(x)
        tr = Track(secs, compressed=comp, plain_bytes=None if t % 2 else max(len(x.plain) for x in secs) + 4 * t + 40)
        if t in (1, 5):     # clip windows that cut items
            a, b = secs[2].leaf[0] + 3, secs[-3].leaf[1] - 3
            tr.clip = (a + 1, b + 1)
        tracks.append(tr)
    return tracks


def test_wavefront_mix(lib, oracle):
    rng = np.random.default_rng(17)
    tracks = _mixed_tracks(rng)
    n_secs = sum(len(t.secs) for t in tracks)
    assert n_secs > 2 * 64
    n = check_mean(lib, oracle, tracks, "mix")
    for t, tr in enumerate(tracks):         # and each track alone, piece for piece
        n += run_one_track(lib, tr, what="mix track %d" % t)
    print("wavefront mix: %d sections, %d runs + pieces" % (n_secs, n))


def test_batch_shapes(lib):
    """Section counts around the wavefront (64), the scan kernel's tiles (1024 x 8) and the resident lanes of one launch
    (bw_fill_sections() + 1); 1..4-item sections of every type; range_lo / range_hi cuts."""
    rng = np.random.default_rng(23)
    p = sum_pipe(lib)
    fill = p.bw_fill_sections()
    assert fill > 0
    p.close()
    counts = [1, 63, 64, 65, 1023, 1024, 8191, 8192, 8193, fill + 1]
    total = 0
    for c in counts:
        secs, pos = [], 5
        for q in range(c):
            x, pos = mk(rng, 0, 1 + q % 3, pos, 1 + q % 4, level=1 + q % 9)
            secs.append(x)
        tr = Track(secs)
        total += run_one_track(lib, tr, what="%d sections" % c)
        s, f, _ = tr.pieces()
        lo, hi = int(s[len(s) // 3]) + 1, int(s[2 * len(s) // 3]) if len(s) > 3 else INT32_MAX
        total += run_one_track(lib, tr, lo, hi, what="%d sections, range" % c)
    print("batch shapes: fill %d, %d pieces" % (fill, total))


# ---------------------------------------------------------------------------------------------------------------------
# e. error bits (streams that inflate cleanly)

def _bad_batches(rng):
    out = []
    # 1: the Adler-32 trailer off by one
    x, pos = mk(rng, 0, 1, 100, 300)
    a = struct.unpack(">I", x.comp[-4:])[0]
    out.append((1, Track([Sec(x.plain, x.comp[:-4] + struct.pack(">I", (a + 1) & 0xFFFFFFFF), x.leaf)])))
    # 2: an item count that does not fit the section's size
    s, e, vb, _ = items(rng, 1, 100, 200)
    plain = section_bytes(0, 1, s, e, vb, count=201)
    out.append((2, Track([Sec(plain, deflate(plain), (int(s[0]), int(e[-1])))])))
    # 4: an item beyond its leaf's extents; items out of order
    x, _ = mk(rng, 0, 1, 100, 200)
    out.append((4, Track([Sec(x.plain, x.comp, (x.leaf[0], x.leaf[1] - 1))])))
    s, e, vb, _ = items(rng, 1, 100, 200)
    s[50], s[51], e[50], e[51] = s[51], s[50], e[51], e[50]
    plain = section_bytes(0, 1, s, e, vb)
    out.append((4, Track([Sec(plain, deflate(plain), (int(s.min()), int(e.max())))])))
    # 8: a coordinate at or above WTAMD_MAX_COORD (clip keeps the batch's extents legal)
    s, e, vb, _ = items(rng, 1, MAX_COORD - 4000, 200)
    plain = section_bytes(0, 1, s, e, vb)
    assert e[-1] >= MAX_COORD
    out.append((8, Track([Sec(plain, deflate(plain))], box=False, clip=(1, MAX_COORD - 8000))))
    return out


def test_error_bits(lib):
    """Each error bit: collect fails, bw_error() names exactly that bit, and the next good batch on the same pipe is
    exact."""
    rng = np.random.default_rng(29)
    from wiggletools_amd import _lib
    good, pos = [], 7
    for q in range(40):
        x, pos = mk(rng, 0, 1 + q % 3, pos, int(rng.integers(1, 2000)), level=q % 10)
        good.append(x)
    good = Track(good)
    p = sum_pipe(lib)
    seen = set()
    for bit, tr in _bad_batches(rng):
        submit(p, [tr])
        with pytest.raises(_lib.WtamdError):
            p.collect()
        assert p.bw_error() == bit, (bit, p.bw_error())
        seen.add(bit)
        p.release()
        submit(p, [good])
        check_one_track(collect_ok(p), good, what="after error bit %d" % bit)
    p.close()
    assert seen == {1, 2, 4, 8}
    print("error bits seen: %s" % sorted(seen))


# ---------------------------------------------------------------------------------------------------------------------
# f. the capacity redo

def test_redo_after_denser_batches(lib):
    """bedGraph batches first (the pipe learns their density: a third of its bound), then fixedStep batches three times
    as dense, several in flight: a later batch overflows run lists sized by density, reports WT_BW_ERR_CAPACITY on
    the device and is decoded again at collect.  Exact either way; on the device pipe the redo must have happened.
    With one decode stream and with two (WTAMD_BW_DECODE_STREAMS=2 is read once per process: see the switches test)."""
    rng = np.random.default_rng(31)
    depth = 3
    p = sum_pipe(lib, depth)
    pending = []
    pos = 10

    def batch(typ, n_secs, n_items):
        nonlocal pos
        secs = []
        for _ in range(n_secs):
            x, pos = mk(rng, 0, typ, pos, n_items, level=1)
            secs.append(x)
        return Track(secs, box=False)
    n = 0

    def feed(plan):
        nonlocal n
        for tr in plan:
            if p.in_flight() >= depth:
                n += check_one_track(collect_ok(p), pending.pop(0), what="redo")
            submit(p, [tr])
            pending.append(tr)
        while pending:
            n += check_one_track(collect_ok(p), pending.pop(0), what="redo")
    feed([batch(1, 8, 2500) for _ in range(2)])                                  # density: a third of the bound
    feed([batch(3, 8, 60000) for _ in range(5)] + [batch(1, 4, 3000)])           # three times as dense, 3 in flight
    redone = p.bw_redone()
    p.close()
    if _backend(lib) == "amd":
        assert redone > 0
    else:
        assert redone == 0
    print("redo: %d batches redone, %d pieces" % (redone, n))


# ---------------------------------------------------------------------------------------------------------------------
# g. switches read once per process: the amd cases again in a fresh child

@pytest.mark.gpu
@pytest.mark.parametrize("env", ["WTAMD_INFLATE_RING=64", "WTAMD_BW_COPY=kernel", "WTAMD_BW_DECODE_STREAMS=2"])
def test_once_per_process_switches_gpu(env):
    k, v = env.split("=")
    e = dict(os.environ, **{k: v})
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-s", "-p", "no:cacheprovider", "-m", "gpu",
                        os.path.join(HERE, "test_bwdev_streams.py"), "-k", "amd and not switches"],
                       cwd=os.path.dirname(HERE), env=e, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (env, r.stdout[-3000:], r.stderr[-2000:])
    assert " passed" in r.stdout and " failed" not in r.stdout


# ---------------------------------------------------------------------------------------------------------------------
# 5. CPU variants of the lane state machine

VARIANTS = {"lead0": ["-DWT_INF_LEAD=0"], "round1": ["-DWT_INF_ROUND=1"], "round3": ["-DWT_INF_ROUND=3"], "round4": ["-DWT_INF_ROUND=4"],
            "lk10_11": ["-DWT_INF_LK1=10", "-DWT_INF_LK2=11"], "lk15_15": ["-DWT_INF_LK1=15", "-DWT_INF_LK2=15"],
            "dk7_9": ["-DWT_INF_DK1=7", "-DWT_INF_DK2=9"], "dk10_12": ["-DWT_INF_DK1=10", "-DWT_INF_DK2=12"]}


def _leading_literal_cases():
    cases = []
    for pre in range(0, 9):
        for period in (1, 2, 3, 4):
            for rep in (3, 4, 7, 8, 9, 15, 16, 17, 40, 258, 259, 600):
                unit = bytes([65 + k for k in range(period)])
                head = bytes([200 + (k * 7) % 50 for k in range(pre)])
                cases.append(head + unit + unit * rep + b"Z" + unit[:1] * 5 + b"qrs")
    return cases


def _check_inflate(inflate, label):
    n = 0
    for trial, raw, comp, is_raw in _streams():
        out = np.zeros(len(raw) + 8, np.uint8)
        got = inflate(comp, len(comp), out.ctypes.data, len(raw), int(is_raw))
        assert got == len(raw) and out[:len(raw)].tobytes() == raw, (label, trial, got, len(raw))
        n += 1
    for i, raw in enumerate(_leading_literal_cases()):
        for level, strategy in ((1, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_RLE), (6, zlib.Z_FIXED)):
            comp = deflate(raw, level, strategy)
            out = np.zeros(len(raw) + 8, np.uint8)
            got = inflate(comp, len(comp), out.ctypes.data, len(raw), 0)
            assert got == len(raw) and out[:len(raw)].tobytes() == raw, (label, i, level, got)
            n += 1
    rng = np.random.default_rng(2)
    for x in _period_sections(rng, list(range(1, 73)) + list(range(248, 261)), levels=(1, 9)) + _match_sections(rng):
        out = np.zeros(len(x.plain) + 8, np.uint8)
        got = inflate(x.comp, len(x.comp), out.ctypes.data, len(x.plain), 0)
        assert got == len(x.plain) and out[:len(x.plain)].tobytes() == x.plain, (label, "geometry", got)
        n += 1
    return n


def _bind_inflate(L, ring):
    L.wtemu_inflate_ring.restype = C.c_longlong
    L.wtemu_inflate_ring.argtypes = [C.c_char_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p]
    return lambda src, n, dst, cap, raw: L.wtemu_inflate_ring(src, n, dst, cap, raw, ring, None)


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_lane_state_machine_variants_equal_zlib(name):
    from emu.build import build_inflate_variant
    L = C.CDLL(build_inflate_variant(name, VARIANTS[name]))
    assert _check_inflate(_bind_inflate(L, 8), name) > 500


def test_lane_state_machine_ring64_equals_zlib():
    """RING = 64 (WTAMD_INFLATE_RING=64): the kernel's second instantiation."""
    from emu.build import build_dropin
    L = C.CDLL(build_dropin())
    assert _check_inflate(_bind_inflate(L, 64), "ring64") > 500
    assert _check_inflate(_bind_inflate(L, 8), "ring8") > 500
