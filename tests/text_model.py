"""The writer's rule in plain Python (wtamd_runs_text, include/wiggletools_amd.h; the reference's printBlock,
src/wigWriter.c:55-119): blocks of 10000 entries, the mode as a last-setter scan, headers, '%f' with the NaN sign, the state
that chains batches, and the compression rule the reference's default writer puts in front (unaryOps.c:235-253).  Also the
cases every test of the text unit shares (cases()), the fixtures recorded from the compiled reference
(tests/golden/text_fixtures.json, written by tests/golden/make_text_golden.py), and the ctypes side of tests/text_emu.cpp."""
import ctypes as C
import hashlib
import json
import math
import os
import struct

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "wiggletools_amd", "csrc")
HEADER = os.path.join(CSRC, "wt_text.h")
BLOCK = 10000
BEDGRAPH = 1
I32_MAX = 2 ** 31 - 1
OK, ERR_ARG, ERR_CAPACITY = 0, 1, 3


def bits_to_float(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def float_to_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def fmt(v):
    """glibc's "%lf" of a double: Python's '%f' (the exact decimal expansion, rounded half to even) with the NaN's sign."""
    if v != v:
        return "-nan" if float_to_bits(v) >> 63 else "nan"
    return "%f" % v


def is_wide(v):
    return v == v and not math.isinf(v) and abs(v) >= 2.0 ** 64


class Lists:
    """A run list as the door takes it: names (n_seg), seg (n_seg + 1 offsets), s / f (int32), v (float64, bit for bit)."""

    def __init__(self, names, seg, s, f, v):
        self.names = [n if isinstance(n, bytes) else n.encode() for n in names]
        self.seg = np.ascontiguousarray(seg, np.int64)
        self.s, self.f = np.ascontiguousarray(s, np.int32), np.ascontiguousarray(f, np.int32)
        self.v = np.ascontiguousarray(v, np.float64)
        assert len(self.seg) == len(self.names) + 1 and self.seg[-1] == len(self.s) == len(self.f) == len(self.v)

    def __len__(self):
        return len(self.s)

    @property
    def n_seg(self):
        return len(self.names)

    def seg_of(self, i):
        return int(np.searchsorted(self.seg, i, side="right")) - 1

    def part(self, a, b):
        """The runs [a, b) with every segment kept (some of them empty)."""
        seg = np.clip(self.seg, a, b) - a
        return Lists(self.names, seg, self.s[a:b], self.f[a:b], self.v[a:b])

    def as_f32(self):
        return Lists(self.names, self.seg, self.s, self.f, self.v.astype(np.float32).astype(np.float64))

    def digest(self):
        h = hashlib.sha256()
        for n in self.names:
            h.update(n + b"\0")
        for x in (self.seg, self.s, self.f, self.v):
            h.update(x.tobytes())
        return h.hexdigest()


def fresh_state():
    return {"in_block": 0, "point_by_point": 0, "last_finish": 0, "continues": 0}


def text(L, flags=0, state=None):
    """(bytes, state after): the rule, one entry after the other."""
    st = dict(state) if state and state["in_block"] > 0 else fresh_state()
    bed = bool(flags & BEDGRAPH)
    out = []
    fresh = True
    for g, name in enumerate(L.names):
        name = name.decode("latin-1")
        for i in range(int(L.seg[g]), int(L.seg[g + 1])):
            s, f, v = int(L.s[i]), int(L.f[i]), float(L.v[i])
            have_prev = st["in_block"] > 0
            same = bool(st["continues"]) if fresh else i > int(L.seg[g])
            pmode = bool(st["point_by_point"]) if have_prev and not bed else False
            ln = f - s
            mode = False if bed else True if ln < 2 else False if ln > 5 else pmode
            val = fmt(v)
            if mode:
                if not have_prev or not pmode or not same or s > st["last_finish"]:
                    out.append("fixedStep chrom=%s start=%d step=1\n" % (name, s))
                out.append((val + "\n") * ln)
            else:
                out.append("%s\t%d\t%d\t%s\n" % (name, s - 1, f - 1, val))
            fresh = False
            st = {"in_block": (st["in_block"] + 1) % BLOCK, "point_by_point": int(mode), "last_finish": f, "continues": 1}
    if len(L) == 0:
        return b"", (dict(state) if state else fresh_state())
    return "".join(out).encode("latin-1"), st


def compress(L):
    """The reference's CompressionWiggleIterator (unaryOps.c:235-253): adjacent runs of one chromosome merge while start ==
    the group's finish and (both NaN or |value - the value of the group's FIRST run| < 1e-6)."""
    names, seg, s, f, v = L.names, [0], [], [], []
    for g in range(len(names)):
        first = len(s)
        for i in range(int(L.seg[g]), int(L.seg[g + 1])):
            a, b, x = int(L.s[i]), int(L.f[i]), float(L.v[i])
            if len(s) > first and a == f[-1] and ((x != x and v[-1] != v[-1]) or abs(x - v[-1]) < 1e-6):
                f[-1] = b
            else:
                s.append(a); f.append(b); v.append(x)
        seg.append(len(s))
    return Lists(names, seg, s, f, v)


def same_lists(A, B):
    return (A.names == B.names and np.array_equal(A.seg, B.seg) and np.array_equal(A.s, B.s) and np.array_equal(A.f, B.f) and
            np.array_equal(A.v.view(np.uint64), B.v.view(np.uint64)))


# ---- the cases ----
def _layout(lengths, gaps, start=1):
    """Runs of the given lengths, gaps[i] base pairs after run i - 1 (gaps[0] after `start`)."""
    s, f, p = [], [], start
    for ln, gp in zip(lengths, gaps):
        p += gp
        s.append(p)
        p += ln
        f.append(p)
    return s, f


def _values(n, k=0):
    """n values, neighbours at least 1/8 apart (the compression rule merges nothing)."""
    return [((i * 37 + k) % 101) / 8.0 - 3.0 + (i % 2) * 0.0625 for i in range(n)]


def special_values():
    vals = [j / 128.0 for j in range(1, 128, 2)]                                    # ties at the sixth decimal
    for k in range(19):
        x = 10.0 ** k - 5e-7
        vals += [float(np.nextafter(x, -np.inf)), x, float(np.nextafter(x, np.inf))]
    vals += [0.0078125, 0.0234375, 9.9999995, 0.9999995, 1.0000005, 0.0, -0.0, -1e-9, 1e-9, 5e-324, -5e-324, 2.2250738585072014e-308, 4.9999995e-7, 5e-7,
             5.000001e-7, 1.5e-6, 2.5e-6, 0.5, 1.0, 123456.789, -0.0078125]
    p53 = 2.0 ** 53
    vals += [p53, float(np.nextafter(p53, 0.0)), float(np.nextafter(p53, np.inf)), -p53, 2.0 ** 52 + 0.5, 2.0 ** 51 + 0.25, 2.0 ** 63, 2.0 ** 64 - 2048.0,
             -(2.0 ** 64 - 2048.0), float(np.float32(2.0 ** 64 - 2.0 ** 40)), 1e19, 9999999999999999999.0]
    vals += [math.inf, -math.inf, bits_to_float(0x7ff8000000000000), bits_to_float(0xfff8000000000000), bits_to_float(0xfff8000000000abc)]
    vals += [1e-45, float(np.float32(1e-45)), float(np.float32(0.1)), float(np.float32(-2.5e-7)), float(np.float32(16777216.0))]
    return vals


def _random_list(seed, n, n_seg=3, names=None):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, 8, n)
    # stretches of short and of long runs, so that the mode changes now and then and holds in between
    long_ = (np.arange(n) // 23) % 3 == 1
    lengths = np.where(long_, rng.integers(2, 40, n), lengths)
    gaps = np.where(rng.random(n) < 0.6, 0, rng.integers(1, 5, n))
    cuts = sorted(rng.choice(np.arange(1, n), n_seg - 1, replace=False).tolist()) if n_seg > 1 else []
    seg = [0] + cuts + [n]
    s, f = [], []
    for a, b in zip(seg[:-1], seg[1:]):
        ss, ff = _layout(lengths[a:b].tolist(), gaps[a:b].tolist())
        s += ss
        f += ff
    return Lists(names or ["chr%d" % (g + 1) for g in range(n_seg)], seg, s, f, _values(n, seed))


def cases():
    """{name: Lists}: every list is one the compression rule leaves alone; each is printed in both modes."""
    out = {}
    # every mode transition with lengths 1 .. 7: enter on 1, hold on 2-5, leave on 6; adjacent, then with gaps
    seq = [3, 1, 2, 3, 4, 5, 1, 6, 2, 7, 1, 1, 5, 6, 6, 1, 7, 4, 1, 2, 6, 3, 1, 5, 4, 3, 2, 1, 7, 7, 2, 1]
    s, f = _layout(seq, [0] * len(seq))
    out["transitions_adjacent"] = Lists(["chr1"], [0, len(seq)], s, f, _values(len(seq)))
    s, f = _layout(seq, [(i * 5) % 3 for i in range(len(seq))])
    out["transitions_gaps"] = Lists(["chrX"], [0, len(seq)], s, f, _values(len(seq), 3))
    # a chromosome change and a gap inside a point-by-point stretch, and exact adjacency (no header); an empty segment between
    seq = [1, 1, 2, 1, 3, 1, 1, 1, 5, 1, 1, 2]
    s1, f1 = _layout(seq[:6], [0, 0, 0, 4, 0, 0], 100)
    s2, f2 = _layout(seq[6:], [0, 0, 0, 1, 0, 0], f1[-1])             # starts where the first chromosome ended: still a header
    out["chrom_change"] = Lists(["chr1", "empty", "chr2"], [0, 6, 6, 12], s1 + s2, f1 + f2, _values(12, 1))
    # a point-by-point stretch that straddles entry 10000: the entry after the seam has L = 3 and prints a bedGraph line
    seq = [7] * 9990 + [1] * 10 + [3] + [2, 1, 1, 4, 1, 6, 1, 1, 1]
    s, f = _layout(seq, [0] * len(seq))
    out["straddle_10000"] = Lists(["chr1"], [0, len(seq)], s, f, _values(len(seq), 2))
    seq = [1] * 10003
    s, f = _layout(seq, [0] * len(seq))
    out["points_across_10000"] = Lists(["chr1", "chr2"], [0, 9999, len(seq)], s, f, _values(len(seq), 5))
    for n in (1, 255, 256, 257, 9999, 10000, 10001, 20001):
        out["random_%d" % n] = _random_list(1000 + n, n, 3 if n > 2 else 1)
    # names of 1 and 255 bytes
    out["names"] = _random_list(77, 300, 2, ["c", "N" * 255])
    # start = 1 prints 0; coordinates at INT32_MAX
    out["coordinates"] = Lists(["chr1", "chr2", "chr3"], [0, 3, 5, 6], [1, 2, 9, I32_MAX - 8, I32_MAX - 1, I32_MAX - 3],
                               [2, 9, 12, I32_MAX - 1, I32_MAX, I32_MAX], [1.5, 2.5, 3.5, 4.5, 5.5, 6.5])
    out["negative_coordinates"] = Lists(["chr1"], [0, 4], [-2 ** 31 + 1, -20, 0, 1], [-2 ** 31 + 2, -10, 1, 9], [1.0, 2.0, 3.0, 4.0])
    # the values: lengths cycle so that each is printed in a bedGraph line and point by point; a gap of 1 keeps them apart
    vals = special_values()
    n = len(vals)
    s, f = _layout([(1, 3, 7)[i % 3] for i in range(n)], [1] * n)
    out["values"] = Lists(["chr1"], [0, n], s, f, vals)
    s, f = _layout([1] * n, [1] * n)
    out["values_points"] = Lists(["chr1"], [0, n], s, f, vals)
    v32 = np.asarray(vals, np.float64).astype(np.float32).astype(np.float64)
    keep = [i for i in range(n) if not is_wide(float(v32[i]))]
    s, f = _layout([(1, 3, 7)[i % 3] for i in range(len(keep))], [1] * len(keep))
    out["values_f32"] = Lists(["chr1"], [0, len(keep)], s, f, v32[keep])
    return out


def wide_lists():
    """[(Lists, n_wide)]: lists with finite values of 2^64 and more."""
    a = cases()["random_257"]
    v = a.v.copy()
    v[200] = 2.0 ** 64
    b = _random_list(5, 10300, 2)
    w = b.v.copy()
    w[3], w[10100], w[10299] = 1.7976931348623157e308, -2.0 ** 64, 1e20
    return [(Lists(a.names, a.seg, a.s, a.f, v), 1), (Lists(b.names, b.seg, b.s, b.f, w), 3)]


def reference_cases():
    """cases() and the wide lists, which only the host sweep prints: what tests/golden/make_text_golden.py records."""
    out = dict(cases())
    for k, (W, _) in enumerate(wide_lists()):
        out["wide_%d" % k] = W
    return out


def refusals():
    """[(name, Lists, flags, state)]: calls the door refuses with WTAMD_ERR_ARG before it writes anything (a name outside 1 ..
    255 bytes apart: test by test, the ctypes side differs)."""
    base = _random_list(9, 10050, 2)

    def with_run(i, s, f):
        ss, ff = base.s.copy(), base.f.copy()
        ss[i], ff[i] = s, f
        return Lists(base.names, base.seg, ss, ff, base.v)

    st = fresh_state()
    return [("unknown flag", base, 2, None), ("unknown flag beside the known one", base, 4 | BEDGRAPH, None),
            ("in_block < 0", base, 0, dict(st, in_block=-1)), ("in_block == 10000", base, 0, dict(st, in_block=BLOCK)),
            ("start == finish", with_run(10020, 7, 7), 0, None), ("start > finish", with_run(3, 9, 8), BEDGRAPH, None),
            ("start == INT32_MIN", with_run(0, -2 ** 31, -2 ** 31 + 1), 0, None)]


def count_refusals():
    """[(name, seg_off, n_seg)]: run counts and offsets the door refuses before it looks at a run -- fewer than 0 or at least
    2^31 runs, offsets that decrease or do not start at 0, a negative number of segments.  The run arrays are those of a small
    three-segment list and are never read; n_seg None: the list's own."""
    return [("2^31 runs", [0, 100, 200, 2 ** 31], None), ("2^31 runs in one segment", [0, 2 ** 31], 1), ("2^40 runs", [0, 1, 2, 2 ** 40], None),
            ("-1 runs", [0, -1], 1), ("a negative offset inside", [0, -5, 100, 255], None), ("offsets decrease", [0, 200, 100, 255], None),
            ("offsets decrease to the list's count", [0, 300, 255, 255], None), ("the first offset is not 0", [1, 100, 200, 255], None),
            ("n_seg < 0", [0, 100, 200, 255], -1)]


def check_count_refusals(door):
    """Every refusal of count_refusals() returns WTAMD_ERR_ARG, in both modes, with the canaries, n_bytes and the state as
    they were.  door(L, flags, state, capacity, offset, seg, n_seg) -> the tuple of call()."""
    L = cases()["random_255"]
    assert L.n_seg == 3
    st0 = {"in_block": 17, "point_by_point": 1, "last_finish": 99, "continues": 1}
    for name, seg, n_seg in count_refusals():
        for flags in (0, BEDGRAPH):
            rc, buf, nb, nw, st = door(L, flags, state=dict(st0), capacity=1 << 16, offset=1, seg=seg, n_seg=n_seg)
            assert rc == ERR_ARG, (name, flags, rc)
            assert (buf == CANARY).all() and st == st0, (name, flags, st)


def cut_points(L):
    """About six cuts: inside a point-by-point stretch, directly before and after entry 10000, between segments, and twice at
    one place (an empty batch)."""
    n = len(L)
    cuts = {n // 3}
    ln = L.f.astype(np.int64) - L.s
    short = np.nonzero((ln[:-1] < 2) & (ln[1:] < 2))[0]
    if len(short):
        cuts.add(int(short[len(short) // 2]) + 1)
    for c in (BLOCK - 1, BLOCK, BLOCK + 1):
        if 0 < c < n:
            cuts.add(c)
    for c in L.seg[1:-1]:
        if 0 < c < n:
            cuts.add(int(c))
    return sorted(cuts)


def chained(door, L, flags, cuts):
    """The list cut at `cuts` and chained through the state, the host flipping `continues` where a cut falls between
    chromosomes: (bytes, state).  door(L, flags, state) -> (rc, bytes, state)."""
    edges = [0] + list(cuts) + [len(L)]
    st = fresh_state()
    out = b""
    last_seg = None
    for a, b in zip(edges[:-1], edges[1:]):
        if b > a:
            st["continues"] = int(last_seg is not None and L.seg_of(a) == last_seg)
        rc, txt, st = door(L.part(a, b), flags, st)
        assert rc == 0, (a, b, rc)
        out += txt
        if b > a:
            last_seg = L.seg_of(b - 1)
    return out, st


# ---- fixtures ----
def fixtures():
    return json.load(open(os.path.join(HERE, "golden", "text_fixtures.json")))["cases"]


def seam_lines(txt, L, flags):
    """The 20 lines on either side of every block seam of the text: [[seam entry, lines before, lines after]]."""
    out = []
    for seam in range(BLOCK, len(L), BLOCK):
        head = text(L.part(0, seam), flags)[0]
        assert txt.startswith(head)
        before = head.decode("latin-1").split("\n")[-21:-1]
        after = txt[len(head):].decode("latin-1").split("\n")[:20]
        out.append([seam, before, after])
    return out


def check_against_fixture(c, L, flags, txt):
    """`txt` is what the compiled reference printed for case c."""
    assert c["input_sha256"] == L.digest(), (c["name"], "the case is not the one recorded")
    assert len(txt) == c["bytes"] and hashlib.sha256(txt).hexdigest() == c["sha256"], (c["name"], flags, len(txt), c["bytes"])
    if "text" in c:
        assert txt == c["text"].encode("latin-1"), (c["name"], flags)
    else:
        assert seam_lines(txt, L, flags) == c["seams"], (c["name"], flags)


# ---- the emulated passes and the host sweep ----
def emu_lib():
    """tests/emu/libwt_text_emu.so, built (tests/emu/build.py) and loaded once."""
    from emu import build
    return build.load_unit("text")


def mergeable_list(n=700, seed=31):
    """A list the compression rule does merge: neighbours that touch and share a value (or are both NaN), in three
    chromosomes; float32-exact values."""
    L = _random_list(seed, n, 3)
    v = np.floor(np.arange(n) / 4.0) / 8.0
    v[50:58] = np.nan
    v[300:303] += [0.0, 2.0 ** -21, 2.0 ** -22]                  # within 1e-6 of the group's first value
    return Lists(L.names, L.seg, L.s, L.f, v)


def constants():
    import re
    txt = open(HEADER).read()
    return {k: int(re.search(r"#define WTX_%s (\d+)\b" % k, txt).group(1)) for k in ("ENTRIES", "WINDOW", "NAME_MAX")}


class State(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("in_block", "point_by_point", "last_finish", "continues")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


CANARY = 0xC7


def call(fn, head, L, flags, state, capacity, offset, tail, names=None, text_ptr=None, seg=None, n_seg=None):
    """One call of a door with HOST arrays: (rc, the whole buffer, n_bytes, n_wide, state after).  The text starts at byte
    `offset` of a buffer of offset + capacity + 64 canary bytes; n_bytes and n_wide start out as -1."""
    names = L.names if names is None else names
    arr = (C.c_char_p * max(len(names), 1))(*names)
    buf = np.full(offset + capacity + 64, CANARY, np.uint8)
    st = State(**state) if state is not None else None
    nb, nw = C.c_int64(-1), C.c_int64(-1)
    p = lambda x: C.c_void_p(x.ctypes.data)      # noqa: E731
    seg = L.seg if seg is None else np.ascontiguousarray(seg, np.int64)
    rc = fn(*head, C.c_int64(len(names) if n_seg is None else n_seg), p(seg), arr, p(L.s), p(L.f), *tail, C.c_uint32(flags), C.byref(st) if st is not None else None,
            C.c_void_p(buf.ctypes.data + offset) if text_ptr is None else text_ptr, C.c_int64(capacity), C.byref(nb), C.byref(nw))
    return rc, buf, nb.value, nw.value, (st.as_dict() if st is not None else None)


def emu_call(L, flags=0, state=None, capacity=None, offset=0, order=0, seed=1, dtype=np.float64, names=None, seg=None, n_seg=None):
    v = np.ascontiguousarray(L.v, dtype)
    cap = len(text(L, flags, state)[0]) if capacity is None else capacity
    fn = emu_lib().text_emu_door
    arr_names = L.names if names is None else names
    arr = (C.c_char_p * max(len(arr_names), 1))(*arr_names)
    buf = np.full(offset + cap + 64, CANARY, np.uint8)
    st = State(**state) if state is not None else None
    nb, nw = C.c_int64(-1), C.c_int64(-1)
    p = lambda x: C.c_void_p(x.ctypes.data)      # noqa: E731
    seg = L.seg if seg is None else np.ascontiguousarray(seg, np.int64)
    rc = fn(C.c_int(order), C.c_uint64(seed), C.c_int64(len(arr_names) if n_seg is None else n_seg), p(seg), arr, p(L.s), p(L.f), p(v), C.c_int(1 if v.dtype == np.float64 else 0),
            C.c_uint32(flags), C.byref(st) if st is not None else None, C.c_void_p(buf.ctypes.data + offset), C.c_int64(cap), C.byref(nb), C.byref(nw), None)
    return rc, buf, nb.value, nw.value, (st.as_dict() if st is not None else None)


def host_call(L, flags=0, state=None, capacity=None, offset=0, names=None, seg=None, n_seg=None, **_):
    cap = len(text(L, flags, state)[0]) if capacity is None else capacity
    return call(emu_lib().text_host, [], L, flags, state, cap, offset, [C.c_void_p(L.v.ctypes.data)], names, seg=seg, n_seg=n_seg)


def payload(buf, offset, n):
    return buf[offset:offset + n].tobytes()


def canaries_intact(buf, offset, n):
    return bool((buf[:offset] == CANARY).all() and (buf[offset + n:] == CANARY).all())


def fmt_c(v):
    """The header's integer "%lf" of one value (None: wide)."""
    fn = emu_lib().text_fmt
    fn.argtypes = [C.c_double, C.c_char_p]
    buf = C.create_string_buffer(40)
    n = fn(C.c_double(v), buf)
    return None if n < 0 else buf.raw[:n].decode()


# ---- checks every door's tests share: door(L, flags, state, capacity, offset, dtype, names) -> the tuple of call() ----
def check_case(door, L, flags, what, dtype=np.float64):
    want, st_want = text(L, flags)
    rc, buf, nb, nw, st = door(L, flags, state=fresh_state(), capacity=len(want), offset=0, dtype=dtype)
    assert (rc, nb, nw) == (0, len(want), 0), (what, rc, nb, nw, len(want))
    got = payload(buf, 0, nb)
    if got != want:
        k = next(i for i in range(min(len(got), len(want))) if got[i] != want[i]) if got[:len(want)] != want[:len(got)] else min(len(got), len(want))
        raise AssertionError((what, "first difference at byte", k, got[max(0, k - 60):k + 60], want[max(0, k - 60):k + 60]))
    assert canaries_intact(buf, 0, nb), what
    if len(L):
        assert st == st_want, (what, st, st_want)
    return got


def check_chained(door, L, flags, what):
    want, st_want = text(L, flags)

    def one(part, fl, st):
        rc, buf, nb, nw, st2 = door(part, fl, state=st, capacity=None, offset=0)
        return rc, payload(buf, 0, nb), st2

    cuts = cut_points(L)
    cuts = sorted(cuts + cuts[:1])                              # one cut twice: an empty batch, which leaves the state alone
    got, st = chained(one, L, flags, cuts)
    assert got == want, (what, cuts)
    assert st == st_want, (what, st, st_want)


def check_alignment_and_capacity(door, L, flags, what):
    want = text(L, flags)[0]
    for off in (0, 1, 2, 3):
        rc, buf, nb, nw, _ = door(L, flags, state=None, capacity=len(want), offset=off)
        assert rc == 0 and payload(buf, off, nb) == want and canaries_intact(buf, off, nb), (what, off)
    rc, buf, nb, nw, st = door(L, flags, state=fresh_state(), capacity=len(want) - 1, offset=1)
    assert rc == ERR_CAPACITY and nb == len(want), (what, rc, nb)
    assert (buf == CANARY).all() and st == fresh_state(), what


def check_refusals(door):
    for name, L, flags, state in refusals():
        rc, buf, nb, nw, st = door(L, flags, state=state if state is not None else fresh_state(), capacity=1 << 20, offset=0)
        assert rc == ERR_ARG, (name, rc)
        assert (buf == CANARY).all(), name
        assert st == (state if state is not None else fresh_state()), name
    L = cases()["random_255"]
    for names in ([b"", b"chr2", b"chr3"], [b"chr1", b"x" * 256, b"chr3"]):
        rc, buf, nb, nw, st = door(L, 0, state=fresh_state(), capacity=1 << 20, offset=0, names=names)
        assert rc == ERR_ARG and (buf == CANARY).all() and st == fresh_state(), names
    for W, n_wide in wide_lists():
        for flags in (0, BEDGRAPH):
            rc, buf, nb, nw, st = door(W, flags, state=fresh_state(), capacity=1 << 22, offset=0)
            assert rc == ERR_ARG and nw == n_wide, (rc, nw, n_wide)
            assert (buf == CANARY).all() and st == fresh_state()
