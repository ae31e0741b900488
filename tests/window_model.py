"""Model of the window operators (tests/test_window_model.py, tests/test_window_gpu.py, tests/golden/make_window_golden.py): a
literal per-pop restatement of the reference's BinningWiggleIterator (src/unaryOps.c:963-1036, `bin`) and SmoothWiggleIterator
(:1039-1162, `smooth`) over an array-backed child, exact (Fraction) wherever they sum; the loaders of the recordings; ctypes
drivers of the plain-C++ passes and host sweeps of csrc/wt_window.h (tests/window_emu.cpp); and the seam cases whose sizes come
from the header's constants.

A value is a float or a Fraction; NaN is the float.  bin() and smooth() return per-pop rows (chromosome index, start, finish,
Term) where Term carries the exact value, the sum of the |terms| that entered it and their number -- what the float bounds of
the tests are made of.  Nothing here normalises a quirk: a gap inside a chromosome reads as 0 under smooth, the trailing phase
drops one value per pop, bin tests the default's truth as C does (NaN counts, -0.0 does not)."""
import ctypes as C
import json
import math
import os
import re
from fractions import Fraction

import numpy as np

from model_common import _p  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "wiggletools_amd", "csrc")
HEADER = os.path.join(CSRC, "wt_window.h")

OK, ERR_ARG, ERR_CAPACITY = 0, 1, 3
DEFAULTS = (0.0, float("nan"), 1.5)
WIDTHS = (2, 3, 7, 10, 64, 100)
INT32_MAX = 2 ** 31 - 1
NAN = float("nan")


def constants():
    """The WWN_* values of csrc/wt_window.h."""
    txt = open(HEADER).read()
    num = lambda name: int(re.search(r"#define WWN_%s (\d+)" % name, txt).group(1))      # noqa: E731
    return {k: num(k) for k in ("TILE", "STRIP", "SMALL", "WAVE", "WINDOW", "RUNS_PER_LANE")}


def isnan(x):
    return isinstance(x, float) and x != x


class Child:
    """An array-backed child by the reference's protocol: chroms = [(start, finish, value)] arrays per chromosome; it holds its
    first element when made, pop() moves on, `chrom` compares by identity (an index here)."""

    def __init__(self, chroms):
        self.chroms, self.c, self.j, self.done = chroms, 0, -1, False
        self.pop()

    def pop(self):
        self.j += 1
        while self.c < len(self.chroms) and self.j >= len(self.chroms[self.c][0]):
            self.c, self.j = self.c + 1, 0
        if self.c >= len(self.chroms):
            self.done = True
            return
        s, f, v = self.chroms[self.c]
        self.chrom, self.start, self.finish, self.value = self.c, int(s[self.j]), int(f[self.j]), v[self.j]


def _exact(v):
    return v if isnan(v) else Fraction(v)


class Term:
    """value: Fraction, or NaN; a: the sum of the |terms|; k: how many there were."""
    __slots__ = ("value", "a", "k")

    def __init__(self, value, a, k):
        self.value, self.a, self.k = value, a, k

    def float(self):
        return NAN if isnan(self.value) else float(self.value)


def cdiv(a, b):
    """C's integer division: towards zero."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def bin(chroms, width, default):
    """BinningWiggleIteratorPop, :978-1025, pop by pop."""
    it = Child(chroms)
    rows = []
    wi_chrom, wi_finish = None, 0
    dflt = _exact(default)
    while not it.done:
        if wi_chrom == it.chrom and it.start < wi_finish + width:                       # :990
            start = wi_finish
        else:
            start = cdiv(it.start - 1, width) * width + 1                                # :994
        wi_chrom, wi_finish = it.chrom, start + width
        value, nan, a, k, total = Fraction(0), False, Fraction(0), 0, 0
        while not it.done and it.chrom == wi_chrom and it.start < wi_finish:            # :1001
            covered = min(it.finish, wi_finish) - max(it.start, start)
            v = _exact(it.value)
            if isnan(v):
                nan = True
            else:
                value, a = value + covered * v, a + abs(covered * v)
            k += 1
            total += covered
            if it.finish > wi_finish:
                break
            it.pop()
        if (isnan(dflt) or dflt != 0) and total < width:                                  # :1023: NaN is true in C
            if isnan(dflt):
                nan = True
            else:
                value, a = value + (width - total) * dflt, a + abs((width - total) * dflt)
            k += 1
        rows.append((wi_chrom, start, wi_finish, Term(NAN if nan else value, a, k)))
    return rows


class _Smooth:
    """The state of SmoothWiggleIteratorData and the three helpers, :1053-1100; the buffer is a ring of `width` slots."""

    def __init__(self, it, width):
        self.it, self.width = it, width
        self.buffer = [Fraction(0)] * width
        self.sum, self.latest, self.oldest, self.last_position, self.count = Fraction(0), 0, 0, 0, 0

    def recompute(self):
        idx = list(range(self.oldest + 1, self.latest)) if self.oldest < self.latest else \
            list(range(self.oldest + 1, self.width)) + list(range(0, self.latest))
        vals = [self.buffer[i] for i in idx]
        return NAN if any(isnan(v) for v in vals) else sum(vals, Fraction(0))

    def erase_one(self):
        if isnan(self.buffer[self.oldest]):
            self.sum = self.recompute()
        elif not isnan(self.sum):
            self.sum -= self.buffer[self.oldest]
        self.count -= 1
        self.oldest += 1
        if self.oldest >= self.width:
            self.oldest = 0

    def read_one(self, chrom, position):
        it = self.it
        while not it.done and it.chrom == chrom and it.finish <= position:
            it.pop()
        if not it.done and it.chrom == chrom:
            if it.start <= position:
                v = _exact(it.value)
                self.buffer[self.latest] = v
                self.sum = NAN if isnan(v) or isnan(self.sum) else self.sum + v
            else:
                self.buffer[self.latest] = Fraction(0)
            self.count += 1
            self.last_position = position
            self.latest += 1
            if self.latest >= self.width:
                self.latest = 0

    def held(self):
        """|values| in the buffer, oldest first."""
        return [self.buffer[(self.oldest + i) % self.width] for i in range(self.count)]


def smooth(chroms, width):
    """SmoothWiggleIteratorPop, :1102-1136, pop by pop.  Term.a: the largest window sum of |values| so far on the chromosome;
    Term.k: the number of values in the window."""
    it = Child(chroms)
    d = _Smooth(it, width)
    rows = []
    chrom, start, peak = None, 0, Fraction(0)
    h = width // 2
    while True:
        if it.done and d.count == 0:
            return rows
        if d.count == 0:
            chrom, start, peak = it.chrom, it.start - h, Fraction(0)
            if start < 1:
                start = 1
                for i in range(h):
                    d.read_one(chrom, start + i)
        else:
            start += 1
        d.read_one(chrom, start + h)
        held = d.held()
        peak = max(peak, sum((abs(v) for v in held if not isnan(v)), Fraction(0)))
        rows.append((chrom, start, start + 1, Term(NAN if isnan(d.sum) else d.sum / width, peak / width, len(held))))
        if d.count == width or d.last_position < start + h:
            d.erase_one()


# ---------------------------------------------------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    """Run lists of several segments: chroms = [(start, finish, value)] with int32 / float64 arrays."""

    def __init__(self, chroms):
        self.chroms = [(np.asarray(s, np.int32), np.asarray(f, np.int32), np.asarray(v, np.float64)) for s, f, v in chroms]
        self.seg = np.concatenate([[0], np.cumsum([len(c[0]) for c in self.chroms])]).astype(np.int64)
        cat = lambda i, dt: np.concatenate([c[i] for c in self.chroms] + [np.zeros(0, dt)]).astype(dt)      # noqa: E731
        self.s, self.f, self.v = cat(0, np.int32), cat(1, np.int32), cat(2, np.float64)

    def values(self, dt):
        out = self.v.astype(dt)
        assert np.array_equal(out.astype(np.float64), self.v, equal_nan=True), "the values must be exact in float32"
        return out

    def only(self, g):
        return Case([self.chroms[g]])


def rows_of(model_rows, n_seg):
    """Model rows -> per segment (start, finish, [Term])."""
    out = [([], [], []) for _ in range(n_seg)]
    for c, s, f, t in model_rows:
        out[c][0].append(s); out[c][1].append(f); out[c][2].append(t)
    return out


def same_bits(a, b):
    """Equal as doubles bit for bit, any NaN equal to any NaN."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


def check_exact(got, model_rows, n_seg, what):
    """got = (seg_off, start, finish, value) of a door; every model value is exact here: bit equality."""
    oseg, os_, of, ov = got
    exp = rows_of(model_rows, n_seg)
    assert len(oseg) == n_seg + 1 and oseg[0] == 0, what
    for g in range(n_seg):
        a, b = int(oseg[g]), int(oseg[g + 1])
        assert os_[a:b].tolist() == exp[g][0] and of[a:b].tolist() == exp[g][1], (what, g)
        assert same_bits(ov[a:b], [t.float() for t in exp[g][2]]), (what, g)
    assert int(oseg[-1]) == len(model_rows), what


# ---- the recordings ----
def load_fixtures():
    return json.load(open(os.path.join(HERE, "golden", "window_fixtures.json")))["cases"]


def _num(x):
    return NAN if x is None else float(x)


def fixture_case(c):
    """(Case, default, width) of a recorded case."""
    seg = c["seg_off"]
    v = np.array([_num(x) for x in c["value"]], np.float64)
    chroms = [(c["start"][a:b], c["finish"][a:b], v[a:b]) for a, b in zip(seg[:-1], seg[1:])]
    return Case(chroms), _num(c["default"]), int(c["width"])


def recorded(rec):
    """A recorded output as [(chromosome, start, finish, value)]: bin rows are stored as they are, smooth rows run-length
    encoded as [chromosome, first position, [value or [value, count], ...]] per island."""
    if "rows" in rec:
        return [(r[0], r[1], r[2], _num(r[3])) for r in rec["rows"]]
    out = []
    for chrom, p, vals in rec["islands"]:
        for x in vals:
            v, n = (x[0], x[1]) if isinstance(x, list) else (x, 1)
            for _ in range(n):
                out.append((chrom, p, p + 1, _num(v)))
                p += 1
    return out


def seek_child(case, g, lo, hi):
    """What the array child of the golden driver delivers after seek(chromosome g, lo, hi): from the first run that ends after
    lo, up to hi, the last run clipped there (the first is not clipped)."""
    s, f, v = case.chroms[g]
    keep = (f > lo) & (s < hi)
    chroms = [(np.zeros(0, np.int32),) * 2 + (np.zeros(0),)] * len(case.chroms)
    chroms[g] = (s[keep], np.minimum(f[keep], hi), v[keep])
    return Case(chroms)


# ---- the plain-C++ passes and host sweeps ----
def emu_lib():
    """tests/emu/libwt_window_emu.so, built (tests/emu/build.py) and loaded once."""
    from emu import build
    return build.load_unit("window")


def _outputs(cap):
    cap = max(int(cap), 1)
    return np.full(cap, -1, np.int32), np.full(cap, -1, np.int32), np.full(cap, -1.0, np.float64)


def bin_capacity(case, width):
    """The bound of the header: the sum over the runs of the bins each touches."""
    s, f = case.s.astype(np.int64), case.f.astype(np.int64)
    return int(((f - 2) // width - (s - 1) // width + 1).sum()) if len(s) else 0


def smooth_capacity(case, width):
    return int(sum(int(f[-1]) - max(1, int(s[0]) - width // 2) + width for s, f, _ in case.chroms if len(s)))


def emu_bin(case, width, default=0.0, dt=np.float64, order=0, seed=0, capacity=None):
    """(rc, n_out, (seg_off, start, finish, value)): the outputs start out as -1 and a refused call leaves them so."""
    v = np.ascontiguousarray(case.v.astype(dt))
    cap = bin_capacity(case, max(width, 1)) if capacity is None else capacity
    os_, of, ov = _outputs(cap)
    oseg, n_out = np.zeros(len(case.seg), np.int64), C.c_int64(-1)
    rc = emu_lib().window_emu_bin(C.c_int(order), C.c_uint64(seed), C.c_int64(len(case.seg) - 1), _p(case.seg), _p(case.s), _p(case.f), _p(v),
                                  C.c_int(int(v.dtype == np.float64)), C.c_int32(width), C.c_double(default), C.c_int64(cap), _p(os_), _p(of), _p(ov),
                                  _p(oseg), C.byref(n_out))
    return rc, n_out.value, (oseg, os_, of, ov)


def emu_smooth(case, width, dt=np.float64, order=0, seed=0, clip=(0, 0), capacity=None):
    v = np.ascontiguousarray(case.v.astype(dt))
    cap = smooth_capacity(case, max(width, 1)) if capacity is None else capacity
    os_, of, ov = _outputs(cap)
    oseg, n_out = np.zeros(len(case.seg), np.int64), C.c_int64(-1)
    rc = emu_lib().window_emu_smooth(C.c_int(order), C.c_uint64(seed), C.c_int64(len(case.seg) - 1), _p(case.seg), _p(case.s), _p(case.f), _p(v),
                                     C.c_int(int(v.dtype == np.float64)), C.c_int32(width), C.c_int32(clip[0]), C.c_int32(clip[1]), C.c_int64(cap),
                                     _p(os_), _p(of), _p(ov), _p(oseg), C.byref(n_out))
    return rc, n_out.value, (oseg, os_, of, ov)


def host_sweep(case, width, default=None, clip=(0, 0)):
    """The host sweeps of the header, segment by segment (default None: smooth): (rc, (seg_off, start, finish, value))."""
    parts, oseg = [], [0]
    for s, f, v in case.chroms:
        one = Case([(s, f, v)])
        cap = bin_capacity(one, width) if default is not None else smooth_capacity(one, width)
        os_, of, ov = _outputs(cap)
        n_out = C.c_int64(-1)
        vv = np.ascontiguousarray(v, np.float64)
        if default is not None:
            rc = emu_lib().window_host_bin(C.c_int64(len(s)), _p(one.s), _p(one.f), _p(vv), C.c_int32(width), C.c_double(default), C.c_int64(cap),
                                           _p(os_), _p(of), _p(ov), C.byref(n_out))
        else:
            rc = emu_lib().window_host_smooth(C.c_int64(len(s)), _p(one.s), _p(one.f), _p(vv), C.c_int32(width), C.c_int32(clip[0]), C.c_int32(clip[1]),
                                              C.c_int64(cap), _p(os_), _p(of), _p(ov), C.byref(n_out))
        if rc != OK:
            return rc, None
        parts.append((os_[:n_out.value], of[:n_out.value], ov[:n_out.value]))
        oseg.append(oseg[-1] + n_out.value)
    cat = lambda i: np.concatenate([p[i] for p in parts]) if parts else np.zeros(0)      # noqa: E731
    return OK, (np.array(oseg, np.int64), cat(0), cat(1), cat(2))


# ---- float bounds ----
def smooth_additions(case_chrom, width, position):
    """m of the issue: the rounded additions the strip scheme performs for an output position -- one per run under the first
    window of the position's strip, then two per step from there (a value enters, a value leaves)."""
    strip = constants()["STRIP"]
    s, f, _ = case_chrom
    h = width // 2
    p0 = max(1, int(s[0]) - h)
    x0 = p0 + (position - p0) // strip * strip
    lo, hi = x0 + h - width + 1, x0 + h
    return int(((f > lo) & (s <= hi)).sum()) + 2 * (position - x0)


def check_bin_bound(got, model_rows, n_seg, what):
    oseg, os_, of, ov = got
    exp = rows_of(model_rows, n_seg)
    for g in range(n_seg):
        a, b = int(oseg[g]), int(oseg[g + 1])
        assert os_[a:b].tolist() == exp[g][0] and of[a:b].tolist() == exp[g][1], (what, g)
        for x, t in zip(ov[a:b], exp[g][2]):
            if isnan(t.value):
                assert x != x, what
            else:
                assert abs(Fraction(float(x)) - t.value) <= (t.k + 2) * Fraction(1, 2 ** 52) * t.a, (what, g, x, float(t.value))


def check_smooth_bound(got, model_rows, case, width, what):
    oseg, os_, of, ov = got
    exp = rows_of(model_rows, len(case.chroms))
    for g in range(len(case.chroms)):
        a, b = int(oseg[g]), int(oseg[g + 1])
        assert os_[a:b].tolist() == exp[g][0] and of[a:b].tolist() == exp[g][1], (what, g)
        for p, x, t in zip(exp[g][0], ov[a:b], exp[g][2]):
            if isnan(t.value):
                assert x != x, what
            else:
                m = smooth_additions(case.chroms[g], width, p)
                assert abs(Fraction(float(x)) - t.value) <= (m + 2) * Fraction(1, 2 ** 53) * t.a, (what, g, p, x, float(t.value))


# ---- generators ----
def runs_from(rng, first, n, lengths, gaps, values=None, nan_share=0.0):
    """n disjoint runs from `first` on: lengths and gaps drawn from the given choices, values k / 8."""
    s, f, pos = [], [], int(first)
    for _ in range(n):
        ln, gp = int(rng.choice(lengths)), int(rng.choice(gaps))
        s.append(pos); f.append(pos + max(ln, 1))
        pos = f[-1] + max(gp, 0)
    v = rng.integers(-80, 80, n) / 8.0 if values is None else np.asarray(values, np.float64)
    if nan_share:
        v = np.where(rng.random(n) < nan_share, np.nan, v)
    return np.array(s, np.int32), np.array(f, np.int32), v


def float_case():
    """About 2000 runs with float32 values that are not dyadic fractions of small integers."""
    rng = np.random.default_rng(77)
    s, f, _ = runs_from(rng, 40, 2000, (1, 2, 3, 5, 9), (0, 0, 1, 4))
    v = rng.standard_normal(2000).astype(np.float32).astype(np.float64) * 100.0
    return Case([(s, f, v.astype(np.float32).astype(np.float64))])


def bin_seams():
    """name -> (Case, width)."""
    c = constants()
    rng = np.random.default_rng(11)
    T, SMALL, WAVE, WINDOW = c["TILE"], c["SMALL"], c["WAVE"], c["WINDOW"]
    out = {}
    empty = ([], [], [])
    ones = lambda n, first=1, gap=0: (first + np.arange(n) * (1 + gap), first + np.arange(n) * (1 + gap) + 1, rng.integers(-80, 80, n) / 8.0)      # noqa: E731
    out["w2"] = (Case([runs_from(rng, 1, 40, (1, 2, 3), (0, 1, 2, 3))]), 2)
    out["first_start_1"] = (Case([runs_from(rng, 1, 9, (1, 4, 7), (0, 6, 7, 8))]), 7)
    out["long_run"] = (Case([([5, 5 + 7 * (3 * T + 5) - 6], [5 + 7 * (3 * T + 5) - 6, 5 + 7 * (3 * T + 5) + 9], [1.25, -3.0])]), 7)
    for n in list(range(SMALL - 1, SMALL + 3)) + list(range(WAVE * SMALL - 1, WAVE * SMALL + 2)):
        w = 2 * n + 10
        out["bin%d" % n] = (Case([ones(3, 1, 1), ones(n, 1 + w + 3, 1), ones(2, 1 + 2 * w, 0)]), w)
    for n in (WINDOW, WINDOW + 1):
        # the first workgroup's TILE bins are owned by exactly n runs: m bins of w one-bp runs each (m w = n - 2), one run that
        # owns the bins m .. TILE - 2, one run in bin TILE - 1; then more bins for a second workgroup
        w = next(w for w in range(2, n) if (n - 2) % w == 0 and (n - 2) // w < T - 1)
        m = (n - 2) // w
        edge = 1 + (T - 1) * w
        s = list(range(1, m * w + 1)) + [m * w + 1, edge] + list(range(edge + 2, edge + 90, 2))
        f = list(range(2, m * w + 2)) + [edge, edge + 1] + list(range(edge + 3, edge + 91, 2))
        out["window%d" % n] = (Case([(s, f, rng.integers(-80, 80, len(s)) / 8.0)]), w)
    out["segments"] = (Case([empty, runs_from(rng, 3, 300, (1, 2, 9), (0, 3, 30)), empty, empty, runs_from(rng, 1, 5, (2,), (1,)), empty]), 10)
    out["nan_runs"] = (Case([runs_from(rng, 2, 200, (1, 2, 9), (0, 3, 30), nan_share=0.2)]), 10)
    return out


def smooth_seams():
    """name -> (Case, width)."""
    c = constants()
    rng = np.random.default_rng(12)
    S = c["STRIP"]
    out = {}
    for w in (2, 3, 4099):
        out["w%d" % w] = (Case([runs_from(rng, 1 + w, 30, (1, 2, 5, 40), (0, 1, 2, 7))]), w)
    for e in (S - 1, S, S + 1, 3 * S + 5, S * 256 - 1, S * 256 + 1):
        out["extent%d" % e] = (Case([runs_from(rng, 50, 1, (e,), (0,)), runs_from(rng, 9, 2, (e // 2 or 1,), (1,))]), 10)
    for w in (4, 7):
        for n in range(1, w + 2):
            out["chrom%d_w%d" % (n, w)] = (Case([([20], [20 + n], [2.5]), ([1], [1 + n], [-0.75])]), w)
    for w in (6, 64, 101):
        h = w // 2
        for s0 in sorted({1, h, h + 1}):
            out["first%d_w%d" % (s0, w)] = (Case([runs_from(rng, s0, 12, (1, 3, w), (0, 2, w + 3))]), w)
        for F in sorted({2, h, h + 1} - {0, 1}):
            out["last%d_w%d" % (F, w)] = (Case([([1], [F], [4.0]), ([max(F - 2, 1)], [F], [1.5])]), w)
    s, f, v = runs_from(rng, 30, 14, (1, 2, 6), (0, 1, 3, 25))
    for k, name in ((0, "entering"), (6, "inside"), (13, "trailing")):
        vv = v.copy()
        vv[k] = np.nan
        out["nan_%s" % name] = (Case([(s, f, vv)]), 10)
    out["gap"] = (Case([([3, 40], [5, 47], [1.0, 2.0])]), 10)
    out["segments"] = (Case([([], [], []), runs_from(rng, 3, 100, (1, 2, 9), (0, 3, 30)), ([], [], []), runs_from(rng, 1, 5, (2,), (1,)), ([], [], [])]), 7)
    return out


def refusals(case):
    """(what, altered Case or None, width) that both doors must refuse with ERR_ARG."""
    g = max(range(len(case.chroms)), key=lambda q: len(case.chroms[q][0]))
    def alt(fn):      # noqa: E306
        chroms = [tuple(np.array(x) for x in c) for c in case.chroms]
        fn(*chroms[g])
        return Case(chroms)
    def unsorted(s, f, v): s[[1, 2]], f[[1, 2]] = s[[2, 1]], f[[2, 1]]      # noqa: E306,E704
    def empty_run(s, f, v): f[1] = s[1]      # noqa: E306,E704
    def zero_start(s, f, v): s[0] = 0      # noqa: E306,E704
    def overlap(s, f, v): f[0] = s[1] + 1      # noqa: E306,E704
    def past(s, f, v): f[-1] = INT32_MAX      # noqa: E306,E704
    return [("width 1", case, 1), ("unsorted", alt(unsorted), 7), ("start >= finish", alt(empty_run), 7), ("start < 1", alt(zero_start), 7),
            ("overlapping", alt(overlap), 7), ("past INT32_MAX", alt(past), 10)]
