"""The Multiplexer writer's rule in plain Python (wtamd_tile_text, include/wiggletools_amd.h; the reference's printBlock,
src/mWigWriter.c:56-133): text_model's blocks, mode scan, headers and '%f', with W values per entry and an optional prefix per
entry.  Also the cases every test of the unit shares (cases()), the fixtures recorded from the compiled reference
(tests/golden/mtext_fixtures.json, written by tests/golden/make_mtext_golden.py), and the ctypes side of tests/mtext_emu.cpp."""
import ctypes as C
import hashlib
import json
import os

import numpy as np

import text_model as tm
from text_model import BEDGRAPH, BLOCK, CANARY, ERR_ARG, ERR_CAPACITY, Lists, State, canaries_intact, cut_points, fmt, fresh_state, payload, special_values  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(tm.CSRC, "wt_mtext.h")
STRICT = 2
MAX_WIDTH = 65536


class Tile:
    """What the door takes: a run list L (its own values unused), vals[n, width] (float64, bit for bit) and, for paste, one
    prefix (bytes) per entry."""

    def __init__(self, L, vals, prefixes=None):
        self.L = L
        self.vals = np.ascontiguousarray(vals, np.float64)
        self.vals = self.vals.reshape(len(L), self.vals.shape[-1] if self.vals.ndim == 2 else max(self.vals.size // max(len(L), 1), 1))
        self.width = self.vals.shape[1]
        self.prefixes = None if prefixes is None else [bytes(p) for p in prefixes]
        assert self.prefixes is None or len(self.prefixes) == len(L)

    def __len__(self):
        return len(self.L)

    def part(self, a, b):
        return Tile(self.L.part(a, b), self.vals[a:b], None if self.prefixes is None else self.prefixes[a:b])

    def prefix_arrays(self):
        """(bytes as uint8, offsets as int64) or (None, None)."""
        if self.prefixes is None:
            return None, None
        off = np.zeros(len(self) + 1, np.int64)
        off[1:] = np.cumsum([len(p) for p in self.prefixes])
        return np.frombuffer(b"".join(self.prefixes) + b"\0", np.uint8).copy(), off

    def digest(self):
        h = hashlib.sha256(self.L.digest().encode())
        h.update(self.vals.tobytes())
        for p in self.prefixes or []:
            h.update(p + b"\n")
        return h.hexdigest()


def row(vals):
    return "".join("\t" + fmt(float(x)) for x in vals) + "\n"


def text(T, flags=0, state=None):
    """(bytes, state after): the rule, one entry after the other."""
    L = T.L
    st = dict(state) if state and state["in_block"] > 0 else fresh_state()
    bed = bool(flags & BEDGRAPH) or T.prefixes is not None
    out = []
    fresh = True
    for g, name in enumerate(L.names):
        name = name.decode("latin-1")
        for i in range(int(L.seg[g]), int(L.seg[g + 1])):
            s, f = int(L.s[i]), int(L.f[i])
            have_prev = st["in_block"] > 0
            same = bool(st["continues"]) if fresh else i > int(L.seg[g])
            pmode = bool(st["point_by_point"]) if have_prev and not bed else False
            ln = f - s
            mode = False if bed else True if ln < 2 else False if ln > 5 else pmode
            r = row(T.vals[i])
            if mode:
                if not have_prev or not pmode or not same or s > st["last_finish"]:
                    out.append("fixedStep chrom=%s start=%d step=1\n" % (name, s))
                out.append(r * ln)
            elif T.prefixes is not None:
                out.append(T.prefixes[i].decode("latin-1") + r)
            else:
                out.append("%s\t%d\t%d%s" % (name, s - 1, f - 1, r))
            fresh = False
            st = {"in_block": (st["in_block"] + 1) % BLOCK, "point_by_point": int(mode), "last_finish": f, "continues": 1}
    if len(L) == 0:
        return b"", (dict(state) if state else fresh_state())
    return "".join(out).encode("latin-1"), st


# ---- the cases ----
def tile_values(seed, n, width):
    """Cells of every length: magnitudes from 1e-3 to 1e11, both signs, some zeros."""
    rng = np.random.default_rng(seed)
    v = (rng.random((n, width)) - 0.3) * 10.0 ** rng.integers(-3, 12, (n, width))
    v[rng.random((n, width)) < 0.05] = 0.0
    return v


def _prefix(i, n):
    return bytes(33 + (i * 7 + k * 13) % 90 for k in range(n))


SMALL_WIDTHS, SMALL_COUNTS, BIG_COUNTS = (1, 2, 3, 63, 64, 65, 257), (1, 255, 256, 257), (9999, 10000, 10001, 20001)
PREFIX_LENGTHS = (0, 1, 15, 16, 17, 20000)

_CASES = None


def cases():
    """{name: Tile}, built once and never changed: each is printed in both modes."""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = {}
    for w in SMALL_WIDTHS:
        for n in SMALL_COUNTS:
            out["w%d_n%d" % (w, n)] = Tile(tm._random_list(2000 + n, n, 3 if n > 2 else 1), tile_values(w * 1000 + n, n, w))
    for n in BIG_COUNTS:                       # the block seams, inside and at the end of the list
        out["w3_n%d" % n] = Tile(tm._random_list(3000 + n, n, 3), tile_values(n, n, 3))
    # rows longer than the emit pass's window (2048 cells of about 10 bytes), L from 1 to 6: up to five copies of such a row
    lengths = [1 + i % 6 for i in range(40)]
    s, f = tm._layout(lengths, [0] * 40)
    out["w2048_n40"] = Tile(Lists(["chr1", "chr2"], [0, 23, 40], s, f, np.zeros(40)), tile_values(7, 40, 2048))
    # every special value in every column of width 5, in a bedGraph line and point by point; the edge of 2^64 is among them
    vals = [v for v in special_values() if not tm.is_wide(v)]
    n = len(vals) * 5
    cells = tile_values(11, n, 5)
    for e in range(n):
        cells[e, e % 5] = vals[e // 5]
    s, f = tm._layout([(1, 3, 7)[i % 3] for i in range(n)], [1] * n)
    out["specials_w5"] = Tile(Lists(["chr1"], [0, n], s, f, np.zeros(n)), cells)
    # the mode's corners: point-by-point runs across entry 10000, a chromosome change, start > the last finish
    base = tm.cases()
    for k, w in (("transitions_adjacent", 2), ("transitions_gaps", 3), ("chrom_change", 2), ("straddle_10000", 2), ("points_across_10000", 2), ("names", 3),
                 ("coordinates", 4), ("negative_coordinates", 2)):
        out["%s_w%d" % (k, w)] = Tile(base[k], tile_values(len(k) + w, len(base[k]), w))
    # paste: prefixes of every length around a 16-byte line, none, and one longer than the window
    L = tm._random_list(41, 300, 2)
    pre = [_prefix(i, PREFIX_LENGTHS[i % 6] if i % 50 < 6 else (i * 11) % 41) for i in range(300)]
    out["paste_w3"] = Tile(L, tile_values(5, 300, 3), pre)
    L = tm._random_list(42, 10001, 2)
    out["paste_w1_n10001"] = Tile(L, tile_values(6, 10001, 1), [_prefix(i, i % 23) for i in range(10001)])
    _CASES = out
    return out


def flags_of(T):
    return (0,) if T.prefixes is not None else (0, BEDGRAPH)


def wide_tiles():
    """[(Tile, n_wide)]: finite cells of 2^64 and more."""
    a = cases()["w3_n257"]
    v = a.vals.copy()
    v[200, 2] = 2.0 ** 64
    b = cases()["w3_n10001"]
    w = b.vals.copy()
    w[3, 0], w[10000, 1], w[10000, 2] = 1.7976931348623157e308, -2.0 ** 64, 1e20
    return [(Tile(a.L, v), 1), (Tile(b.L, w), 3)]


def reference_cases():
    """What tests/golden/make_mtext_golden.py records: cases() the reference can be given -- paste lines fit its 5000-byte
    buffer -- and the wide tiles, which only the host sweep prints."""
    out = {k: T for k, T in cases().items() if T.prefixes is None or max(len(p) for p in T.prefixes) < 4999}
    for k, (W, _) in enumerate(wide_tiles()):
        out["wide_%d" % k] = W
    return out


def refusals():
    """[(name, Tile, keywords of the door)]: calls refused with WTAMD_ERR_ARG before anything is written."""
    T = cases()["w3_n257"]
    P = cases()["paste_w3"]
    st = fresh_state()

    def with_run(i, s, f):
        ss, ff = T.L.s.copy(), T.L.f.copy()
        ss[i], ff[i] = s, f
        return Tile(Lists(T.L.names, T.L.seg, ss, ff, T.L.v), T.vals)

    return [("width 0", T, dict(width=0)), ("width above the maximum", T, dict(width=MAX_WIDTH + 1)), ("width < 0", T, dict(width=-3)),
            ("prefix without prefix_off", P, dict(prefix_mode="prefix")), ("prefix_off without prefix", P, dict(prefix_mode="off")),
            ("unknown flag", T, dict(flags=4)), ("the track set's flag", T, dict(flags=STRICT)),
            ("in_block < 0", T, dict(state=dict(st, in_block=-1))), ("in_block == 10000", T, dict(state=dict(st, in_block=BLOCK))),
            ("start == finish", with_run(200, 7, 7), {}), ("start > finish", with_run(3, 9, 8), dict(flags=BEDGRAPH)),
            ("start == INT32_MIN", with_run(0, -2 ** 31, -2 ** 31 + 1), {})]


# ---- fixtures ----
def fixtures():
    return json.load(open(os.path.join(HERE, "golden", "mtext_fixtures.json")))


def seam_lines(txt, T, flags):
    """The 20 lines on either side of every block seam of the text: [[seam entry, lines before, lines after]]."""
    out = []
    for seam in range(BLOCK, len(T), BLOCK):
        head = text(T.part(0, seam), flags)[0]
        assert txt.startswith(head)
        out.append([seam, head.decode("latin-1").split("\n")[-21:-1], txt[len(head):].decode("latin-1").split("\n")[:20]])
    return out


# ---- the emulated passes and the host sweep ----
_LIB = None


def emu_lib():
    """tests/emu/libwt_mtext_emu.so (tests/mtext_emu.cpp), built by tests/emu/build.py's build_lib and loaded once."""
    global _LIB
    if _LIB is None:
        from emu import build
        _LIB = C.CDLL(build.build_lib(os.path.join(build.HERE, "libwt_mtext_emu.so"), [os.path.join(HERE, "mtext_emu.cpp")], libs=["-lm"]))
    return _LIB


def call(fn, head, T, flags=0, state=None, capacity=None, offset=0, width=None, prefix_mode="both", names=None, **_):
    """One call of a door with HOST arrays: (rc, the whole buffer, n_bytes, n_wide, state after).  The text starts at byte
    `offset` of a buffer of offset + capacity + 64 canary bytes (capacity None: what the model needs); n_bytes and n_wide start
    out as -1.  prefix_mode "prefix" / "off": only that one of the two is given."""
    L = T.L
    names = L.names if names is None else names
    arr = (C.c_char_p * max(len(names), 1))(*names)
    cap = len(text(T, flags, state)[0]) if capacity is None else capacity
    buf = np.full(offset + cap + 64, CANARY, np.uint8)
    st = State(**state) if state is not None else None
    nb, nw = C.c_int64(-1), C.c_int64(-1)
    p = lambda x: C.c_void_p(x.ctypes.data) if x is not None else None      # noqa: E731
    pre, off = T.prefix_arrays()
    if prefix_mode == "prefix":
        off = None
    if prefix_mode == "off":
        pre = None
    rc = fn(*head, C.c_int64(len(names)), p(L.seg), arr, p(L.s), p(L.f), p(T.vals), C.c_int32(T.width if width is None else width), p(pre), p(off),
            C.c_uint32(flags), C.byref(st) if st is not None else None, C.c_void_p(buf.ctypes.data + offset), C.c_int64(cap), C.byref(nb), C.byref(nw))
    return rc, buf, nb.value, nw.value, (st.as_dict() if st is not None else None)


def emu_call(T, order=0, seed=1, **kw):
    fn = emu_lib().mtext_emu_door
    fn.restype = C.c_int
    rc, buf, nb, nw, st = call(lambda *a: fn(*a, None), [C.c_int(order), C.c_uint64(seed)], T, **kw)
    return rc, buf, nb, nw, st


def host_call(T, **kw):
    return call(emu_lib().mtext_host, [], T, **kw)


# ---- checks every door's tests share: door(T, flags=, state=, capacity=, offset=, width=, prefix_mode=, names=) -> the tuple of call() ----
_WANT = {}


def want(name, flags):
    """The model's (bytes, state) of a case, computed once."""
    if (name, flags) not in _WANT:
        _WANT[(name, flags)] = text(cases()[name], flags)
    return _WANT[(name, flags)]


def first_difference(got, expect):
    k = next((i for i in range(min(len(got), len(expect))) if got[i] != expect[i]), min(len(got), len(expect)))
    return ("first difference at byte", k, got[max(0, k - 60):k + 60], expect[max(0, k - 60):k + 60])


def check_case(door, name, flags):
    T = cases()[name]
    expect, st_expect = want(name, flags)
    rc, buf, nb, nw, st = door(T, flags=flags, state=fresh_state(), capacity=len(expect), offset=0)
    assert (rc, nb, nw) == (0, len(expect), 0), (name, flags, rc, nb, nw, len(expect))
    got = payload(buf, 0, nb)
    assert got == expect, (name, flags) + first_difference(got, expect)
    assert canaries_intact(buf, 0, nb), name
    assert st == st_expect, (name, st, st_expect)
    return got


def check_chained(door, name, flags):
    T = cases()[name]
    expect, st_expect = want(name, flags)

    def one(part, fl, st):
        rc, buf, nb, nw, st2 = door(T.part(*part), flags=fl, state=st, capacity=None, offset=0)
        return rc, payload(buf, 0, nb), st2

    class Parts:                                # text_model.chained cuts through part(a, b): hand it the bounds
        seg = T.L.seg
        seg_of = T.L.seg_of

        def __len__(self):
            return len(T)

        def part(self, a, b):
            return (a, b)

    cuts = cut_points(T.L)
    cuts = sorted(cuts + cuts[:1])              # one cut twice: an empty batch, which leaves the state alone
    got, st = tm.chained(one, Parts(), flags, cuts)
    assert got == expect, (name, cuts) + first_difference(got, expect)
    assert st == st_expect, (name, st, st_expect)


def check_alignment_and_capacity(door, name, flags, offsets=range(16)):
    T = cases()[name]
    expect = want(name, flags)[0]
    for off in offsets:
        rc, buf, nb, nw, _ = door(T, flags=flags, state=None, capacity=len(expect), offset=off)
        assert rc == 0 and payload(buf, off, nb) == expect and canaries_intact(buf, off, nb), (name, off)
    rc, buf, nb, nw, st = door(T, flags=flags, state=fresh_state(), capacity=len(expect) - 1, offset=1)
    assert rc == ERR_CAPACITY and nb == len(expect), (name, rc, nb)
    assert (buf == CANARY).all() and st == fresh_state(), name


def check_refusals(door):
    for name, T, kw in refusals():
        kw = dict(dict(flags=0, state=fresh_state()), **kw)
        rc, buf, nb, nw, st = door(T, capacity=1 << 20, offset=0, **kw)
        assert rc == ERR_ARG, (name, rc)
        assert (buf == CANARY).all(), name
        assert st == kw["state"], name
    for W, n_wide in wide_tiles():
        for flags in (0, BEDGRAPH):
            rc, buf, nb, nw, st = door(W, flags=flags, state=fresh_state(), capacity=1 << 22, offset=0)
            assert rc == ERR_ARG and nw == n_wide, (rc, nw, n_wide)
            assert (buf == CANARY).all() and st == fresh_state()
