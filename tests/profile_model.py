"""Model of the region profiles (csrc/wt_profile.h, wtamd_runs_profile: the reference's `profile` / `profiles`,
ProfileMultiplexer of src/apply.c over regionProfile of src/plots.c) and the helpers the profile tests share.

literal(): the reference's rule, base pair by base pair -- the buffered runs (one 1-bp run per covered position, ONE run per
maximal uncovered stretch with the default), start = round(a c), finish = round(b c) with C's round (libm through ctypes) on
the double product, finish <= start -> start + 1, finish > W -> W, v / (finish - start) to every bin of [start, finish).
closed(): the same through b_j = the smallest i in [0, L] with round(i c) >= j and the gap rule; tested equal to literal().

Per bin both return (sum, sum of |terms|, number of terms k, ok) with the terms taken as the reference's own doubles (v, or the
rounded quotient v / n), accumulated in Fraction; ok: every term is a multiple of 2^-10.  A bin is `exact` when ok and
sum of |terms| < 2^40: then any order of double additions, and len * v in place of v added len times, gives the exact sum.
check(): bit equality where exact, otherwise |got - sum| <= (k + 2) 2^-52 sum of |terms| -- the standard bound of a
floating-point sum of k terms in any order (each of the at most k + 1 roundings, one more for a len * v product, is relative
2^-53 of a partial sum that never exceeds sum of |terms| (1 + k 2^-53))."""
import ctypes as C
import ctypes.util
import json
import os
import re
from fractions import Fraction

import numpy as np

import apply_model as AM
from model_common import _p  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "wiggletools_amd", "csrc")
HEADER = os.path.join(CSRC, "wt_profile.h")

OK, ERR_ARG = 0, 1
SUM = 1
DEFAULTS = (0.0, 1.5, float("nan"))
U = Fraction(1, 1 << 52)

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.round.restype = C.c_double
_libm.round.argtypes = [C.c_double]


def cround(x):
    """C's round (halves away from zero)."""
    return _libm.round(float(x))


def cround_vec(x):
    """The same over a non-negative array: x - floor(x) is exact, so the comparison with 0.5 is."""
    fl = np.floor(x)
    return fl + (x - fl >= 0.5)


def constants():
    """The WPR_* values of csrc/wt_profile.h next to those of wt_apply.h."""
    txt = open(HEADER).read()
    num = lambda name: int(re.search(r"#define %s (\d+)" % name, txt).group(1))      # noqa: E731
    c = dict(AM.constants())
    c.update({"SMALL": num("WPR_SMALL"), "WAVE": num("WPR_WAVE"), "FOLD": num("WPR_FOLD"),
              "BATCH_DOUBLES": 1 << int(re.search(r"#define WPR_BATCH_DOUBLES \(1ll << (\d+)\)", txt).group(1))})
    return c


class Bin:
    __slots__ = ("s", "a", "k", "ok")

    def __init__(self):
        self.s, self.a, self.k, self.ok = Fraction(0), Fraction(0), 0, True

    def add(self, term, times=1):
        t = Fraction(term)
        self.s += t * times
        self.a += abs(t) * times
        self.k += times
        if (t * 1024).denominator != 1:
            self.ok = False

    def merge(self, o):
        self.s += o.s
        self.a += o.a
        self.k += o.k
        self.ok = self.ok and o.ok

    @property
    def exact(self):
        return self.ok and self.a < (1 << 40)


def _clip(s, f, v, rs, rf):
    """The runs of a sorted disjoint segment under [rs, rf), relative to rs."""
    ps, pf, pv = AM.pieces(s, f, v, rs, rf)
    return (ps - rs).astype(np.int64), (pf - rs).astype(np.int64), pv


def literal(s, f, v, rs, rf, W, default):
    """[Bin] * W, base pair by base pair."""
    L = int(rf) - int(rs)
    c = W / float(L)
    ps, pf, pv = _clip(s, f, v, rs, rf)
    isset, val = np.zeros(L, bool), np.zeros(L)
    for a, b, x in zip(ps, pf, pv):
        isset[a:b], val[a:b] = True, x
    bins = [Bin() for _ in range(W)]
    i = 0
    while i < L:
        a = i
        if isset[i]:
            x = float(val[i])
            i += 1
        else:
            x = float(default)
            while i < L and not isset[i]:
                i += 1
        if x != x:
            continue
        st, fi = int(cround(a * c)), int(cround(i * c))
        if fi <= st:
            fi = st + 1
        if fi > W:
            fi = W
        for p in range(st, fi):
            bins[p].add(x / (fi - st))
    return bins


def closed(s, f, v, rs, rf, W, default):
    """[Bin] * W through b_j and the gap rule."""
    L = int(rf) - int(rs)
    c = W / float(L)
    r = cround_vec(np.arange(L + 1, dtype=np.float64) * c).astype(np.int64)
    b = np.searchsorted(r, np.arange(W + 2), side="left")          # in [0, L + 1]
    ps, pf, pv = _clip(s, f, v, rs, rf)
    ends = np.concatenate([[0], pf])
    begins = np.concatenate([ps, [L]])
    gaps = [(int(x), int(y)) for x, y in zip(ends, begins) if y > x]
    ga = np.array([g[0] for g in gaps], np.int64)

    def width_of(x, y):
        fin = min(max(int(r[y]), int(r[x]) + 1), W)
        return fin - int(r[x])

    bins = [Bin() for _ in range(W)]
    d = float(default)
    for j in range(W):
        bj, bj1 = int(b[j]), int(b[j + 1])
        p1 = min(bj1, L)
        p0 = min(bj if bj < bj1 else bj - 1, L)
        k0, k1 = int(np.searchsorted(pf, p0, side="right")), int(np.searchsorted(ps, p1, side="left"))
        for q in range(k0, k1):
            x = float(pv[q])
            u, w = max(int(ps[q]), p0), min(int(pf[q]), p1)
            if x != x or w <= u:
                continue
            if w == p1:
                if w - u > 1:
                    bins[j].add(x, w - u - 1)
                bins[j].add(x / width_of(p1 - 1, p1))
            else:
                bins[j].add(x, w - u)
        if d == d and len(gaps):
            # the gaps that start inside [b_j, b_{j+1}), and the one before them that may span the bin
            g0 = max(int(np.searchsorted(ga, bj, side="left")) - 1, 0)
            for x, y in gaps[g0:int(np.searchsorted(ga, bj1, side="left"))]:
                if x < bj1 and (y >= bj1 or x >= bj):
                    bins[j].add(d / width_of(x, y))
    return bins


def same_bins(a, b):
    return len(a) == len(b) and all(x.s == y.s and x.a == y.a and x.k == y.k and x.ok == y.ok for x, y in zip(a, b))


def check_row(got, bins, what=""):
    """One row of an implementation (device, emulator, host sweep) against the model's bins."""
    assert len(got) == len(bins), (what, len(got), len(bins))
    for j, (g, m) in enumerate(zip(got, bins)):
        g = float(g)
        if m.exact:
            assert g == float(m.s), (what, j, g, float(m.s))
        else:
            assert g == g and abs(Fraction(g) - m.s) <= (m.k + 2) * U * m.a, (what, j, g, float(m.s), m.k, float(m.a))


def column_sums(rows):
    """The model of the sum mode: per column, the concatenated terms of every row."""
    out = [Bin() for _ in rows[0]]
    for row in rows:
        for o, m in zip(out, row):
            o.merge(m)
    return out


class Expected:
    """The model's rows of a Case (apply_model.Case) per (width, default), computed once."""

    def __init__(self, case, model=closed):
        self.case, self.model, self._rows = case, model, {}

    def rows(self, W, default):
        key = (int(W), "nan" if default != default else repr(float(default)))
        if key not in self._rows:
            out = []
            for (s, f, v), (rs_, rf_) in zip(self.case.data, self.case.regions):
                for a, b in zip(rs_, rf_):
                    out.append(self.model(s, f, v, int(a), int(b), int(W), default))
            self._rows[key] = out
        return self._rows[key]

    def check(self, got, W, default, what="", sum_mode=False):
        rows = self.rows(W, default)
        if sum_mode:
            assert got.shape == (W,), (what, got.shape)
            if rows:
                check_row(got, column_sums(rows), what)
            else:
                assert not got.any(), what
            return
        assert got.shape == (len(rows), W), (what, got.shape, len(rows))
        for i, row in enumerate(rows):
            check_row(got[i], row, (what, i))

    def inexact_share(self, W, default):
        bins = [m for row in self.rows(W, default) for m in row]
        return sum(not m.exact for m in bins), len(bins)


same_rows = AM.same_rows


# ---- case builders ----
def _reg(pairs):
    return np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)


def cover(rng, span, exact_sum=True, nan_prob=0.05, gap_prob=0.3, max_len=8):
    """A dataset over [0, span) and a little beyond: runs of length 1 .. max_len, gaps among them."""
    n = max(2 * span // (max_len + 1) + 4, 4)
    s, f, v = AM.dataset(rng, n, exact_sum, nan_prob=nan_prob, gap_prob=gap_prob)
    return s, f, v


ROUNDING = [(8, 4), (64, 32), (7, 7), (64, 64), (8, 7), (6, 7), (65, 64), (63, 64), (15, 7), (13, 7), (129, 64), (127, 64), (20, 4),
            (37, 1), (1, 1), (1, 5), (3, 4099), (999983, 1000), (1000, 3), (10, 100)]       # (L, W)


def rounding_cases():
    """{name: (Case, W)}: one region of length L over a dataset with gaps and NaN runs, another shifted into it, and the
    issue's two worked examples."""
    rng = np.random.default_rng(31)
    out = {}
    for L, W in ROUNDING:
        d = cover(rng, L + 12, max_len=8 if L < 10000 else 900)
        regs = sorted({(3, 3 + L), (5, 5 + L), (int(d[1][1]), int(d[1][1]) + L)})
        out["L%d_W%d" % (L, W)] = (AM.Case([d], [_reg(regs)], True), W)
    ones = (np.array([0], np.int32), np.array([40], np.int32), np.array([1.0]))
    out["ones"] = (AM.Case([ones], [_reg([(10, 30)])], True), 4)
    two = (np.array([102, 110], np.int32), np.array([105, 118], np.int32), np.array([2.0, 1.0]))
    out["worked"] = (AM.Case([two], [_reg([(100, 120)])], True), 4)
    return out


def regime_cases():
    """{name: (Case, W)} at the sizes where the passes change path."""
    c = constants()
    S, WV, T, WIN = c["SMALL"], c["WAVE"], c["TILE"], c["WINDOW"]
    rng = np.random.default_rng(32)
    out = {}
    empty_d = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    empty_r = (np.zeros(0, np.int32), np.zeros(0, np.int32))
    # n runs under ONE bin (W = 1: every position with round(i c) == 0, the first half of the region), exact and float values
    for n in (S - 1, S, S + 1, S + 2, WV - 1, WV, WV + 1, S * WV - 1, S * WV, S * WV + 1, 3 * S * WV + 5):
        for ex in (True, False):
            d = AM.dataset(rng, 2 * n + 40, ex, nan_prob=0.1, gap_prob=0.2)
            rs = int(d[0][5]) + 1
            end = int(d[1][5 + n - 1]) - (1 if d[1][5 + n - 1] - d[0][5 + n - 1] > 1 else 0)       # the last position of bin 0 is in run 5 + n - 1
            # bin 0 of W = 2 holds the positions with round(2 i / L) == 0: i < L / 4
            L = 4 * (end - rs)
            case = AM.Case([d], [_reg([(rs, rs + L), (rs, rs + L), (rs + 1, rs + 1 + L)])], ex)
            out["bin%d%s" % (n, "" if ex else "_float")] = (case, 2)
    # T - 1 .. 3 T + 5 regions
    for n in (T - 1, T, T + 1, 3 * T + 5):
        d = AM.dataset(rng, n // 2, True, nan_prob=0.05)
        out["regions%d" % n] = (AM.Case([d], [AM.random_regions(rng, d, n, 6)], True), 3)
    # one tile whose dataset window is exactly WIN, and WIN + 1, runs
    for w in (WIN, WIN + 1):
        d = AM.dataset(rng, w + 30, True, nan_prob=0.02)
        first, last = AM.over_runs(d, 11, 14), AM.over_runs(d, 11 + w - 5, 11 + w)
        a = np.sort(rng.integers(12, 11 + w - 6, 60))
        b = np.minimum(a + rng.integers(1, 7, len(a)), 11 + w - 1)
        rs = np.concatenate([[first[0]], d[0][a], [last[0]]])
        rf = np.concatenate([[first[1]], d[1][b - 1], [last[1]]])
        assert (np.diff(rs) >= 0).all() and rf.max() == last[1] and (rf > rs).all()
        out["window%d" % w] = (AM.Case([d], [(rs.astype(np.int32), rf.astype(np.int32))], True), 5)
    # several segments in one tile, empty ones on either side
    ds = [AM.dataset(rng, k, True, nan_prob=0.1) for k in (40, 7, 90, 3)]
    out["segments"] = (AM.Case([empty_d, ds[0], empty_d, ds[1], empty_d, ds[2], empty_d, ds[3], empty_d],
                               [empty_r, AM.random_regions(rng, ds[0], 20, 9), _reg([(3, 9), (5, 50)]), empty_r, empty_r,
                                AM.random_regions(rng, ds[2], 50, 40), empty_r, AM.random_regions(rng, ds[3], 4, 3), _reg([(1, 9)])]), 7)
    # spelled out: runs [10,20) = 1, [20,25) = NaN, [30,40) = -0.0, [40,41) = 0.25, [50,60) = 2.5
    d = (np.array([10, 20, 30, 40, 50], np.int32), np.array([20, 25, 40, 41, 60], np.int32), np.array([1.0, np.nan, -0.0, 0.25, 2.5]))
    regs = [(1, 5), (1, 10), (1, 11), (5, 70), (10, 20), (12, 18), (12, 18), (19, 21), (20, 25), (20, 30), (25, 30), (26, 29), (30, 41), (39, 52),
            (40, 41), (41, 50), (41, 100), (59, 60), (60, 61), (60, 900), (70, 80)]
    for W in (1, 3, 4, 10, 64):       # a region with no data, one inside one run, gaps over several bins, a gap into the dropped tail
        out["edges_W%d" % W] = (AM.Case([d], [_reg(regs)], True), W)
    return out


def float_case():
    """2 000 float runs, 300 random regions and one region over all of it."""
    rng = np.random.default_rng(33)
    d = AM.dataset(rng, 2000, False, nan_prob=0.01)
    rs, rf = AM.random_regions(rng, d, 300, 60)
    rs = np.concatenate([[0], rs]).astype(np.int32)
    rf = np.concatenate([[int(d[1][-1]) + 5], rf]).astype(np.int32)
    return AM.Case([d], [(rs, rf)], False)


def refusals(case):
    """[(what, keyword changes)] every door refuses (shared with the device's test)."""
    s, f, rs, rf, seg = case.s, case.f, case.rs, case.rf, case.seg
    a = int(seg[1])                                                   # inside the first non-empty dataset segment
    s2 = s.copy(); s2[a + 5], s2[a + 6] = s[a + 6], s[a + 5]          # dataset not sorted
    f3 = f.copy(); f3[a + 9] = s[a + 9]                               # an empty dataset run
    f4 = f.copy(); f4[a + 3] = s[a + 4] + 1                           # dataset runs overlap
    rs2 = rs.copy(); rs2[2], rs2[3] = max(rs[2], rs[3]) + 1, min(rs[2], rs[3])
    rf2 = np.maximum(rf, rs2 + 1)                                     # regions not sorted
    rf3 = rf.copy(); rf3[4] = rs[4]                                   # an empty region
    s5 = s.copy(); s5[0] = -1                                         # a negative start, either side
    rs5 = rs.copy(); rs5[0] = -1
    return [("unsorted dataset", dict(s=s2)), ("empty run", dict(f=f3)), ("overlapping dataset", dict(f=f4)), ("unsorted regions", dict(rs=rs2, rf=rf2)),
            ("empty region", dict(rf=rf3)), ("negative dataset start", dict(s=s5)), ("negative region start", dict(rs=rs5)),
            ("width 0", dict(W=0)), ("width -3", dict(W=-3)), ("unknown flag", dict(flags=2)), ("unknown flag with sum", dict(flags=5))]


def altered(case, s=None, f=None, rs=None, rf=None):
    k = AM.Case(case.data, case.regions, True)
    k.s, k.f = (case.s if s is None else s), (case.f if f is None else f)
    k.rs, k.rf = (case.rs if rs is None else rs), (case.rf if rf is None else rf)
    return k


# ---- the passes of csrc/wt_profile.h on the CPU (tests/profile_emu.cpp) ----
def emu_lib():
    """tests/emu/libwt_profile_emu.so, built (tests/emu/build.py) and loaded once."""
    from emu import build
    return build.load_unit("profile")


def _out(case, W, flags):
    n = 1 if flags & SUM else max(len(case.rs), 1)
    return np.full((n, max(int(W), 1)), -1.0)


def _shape(out, case, W, flags):
    return out[0] if flags & SUM else out[:len(case.rs)]


def emu_case(case, W, default=0.0, flags=0, dt=np.float64, order=0, seed=0, batch=0):
    """Returns (rc, rows or the sum); the output starts out filled with -1 and a refused call leaves it so."""
    v = np.ascontiguousarray(case.values(dt))
    out = _out(case, W, flags)
    rc = emu_lib().profile_emu(C.c_int(order), C.c_uint64(seed), C.c_int64(len(case.seg) - 1), _p(case.seg), _p(case.s), _p(case.f), _p(v),
                               C.c_int(int(v.dtype == np.float64)), _p(case.rseg), _p(case.rs), _p(case.rf), C.c_int32(W), C.c_double(default),
                               C.c_uint32(flags), C.c_int64(batch), _p(out))
    return rc, _shape(out, case, W, flags)


def host_sweep(case, W, default=0.0):
    """The host sweep of csrc/wt_profile.h, segment pair by segment pair: (rc, rows)."""
    out = np.full((max(len(case.rs), 1), W), -1.0)
    for g in range(len(case.seg) - 1):
        a, b, ra, rb = int(case.seg[g]), int(case.seg[g + 1]), int(case.rseg[g]), int(case.rseg[g + 1])
        s, f, v = (np.ascontiguousarray(x[a:b]) for x in (case.s, case.f, case.v))
        rs, rf = np.ascontiguousarray(case.rs[ra:rb]), np.ascontiguousarray(case.rf[ra:rb])
        part = np.full((max(rb - ra, 1), W), -1.0)
        rc = emu_lib().profile_host(C.c_int64(b - a), _p(s), _p(f), _p(v), C.c_int64(rb - ra), _p(rs), _p(rf), C.c_int32(W), C.c_double(default),
                                    C.c_uint32(0), _p(part))
        if rc != 0:
            return rc, out[:0]
        out[ra:rb] = part[:rb - ra]
    return 0, out[:len(case.rs)]


def host_sum(case, W, default=0.0):
    """The host sweep's sum mode over a case of ONE segment."""
    assert len(case.seg) == 2
    out = np.full(W, -1.0)
    rc = emu_lib().profile_host(C.c_int64(len(case.s)), _p(case.s), _p(case.f), _p(np.ascontiguousarray(case.v)), C.c_int64(len(case.rs)), _p(case.rs),
                                _p(case.rf), C.c_int32(W), C.c_double(default), C.c_uint32(SUM), _p(out))
    return rc, out


# ---- the recordings of the compiled reference (tests/golden/profile_fixtures.json) ----
def load_fixtures():
    return json.load(open(os.path.join(HERE, "golden", "profile_fixtures.json")))["cases"]


def fixture_case(c):
    """(Case, default, width) of a recorded case; regions in the order the reference served them."""
    case, default = AM.fixture_case(c)
    return case, default, int(c["width"])


def recorded_rows(c):
    """The recorded rows; the file holds a value, or [value, count] for count equal consecutive bins."""
    num = lambda x: float("nan") if x is None else float(x)      # noqa: E731
    rows = [[num(v) for x in row for v in ([x[0]] * x[1] if isinstance(x, list) else [x])] for row in c["rows"]]
    return np.array(rows, np.float64).reshape(-1, int(c["width"]))
