"""The rule of wtamd_runs_histogram (include/wiggletools_amd.h, csrc/wt_hist.h) as a NumPy model, the printed forms of the
reference's print_histogram / normalize_histogram (src/plots.c:196-223), the recorded fixtures
(tests/golden/hist_fixtures.json), ctypes drivers of the emulated passes and the host sweep (tests/hist_emu.cpp), and the seam
cases whose sizes come from the header's constants -- shared by tests/test_hist_model.py, test_hist_emu.py, test_hist_gpu.py,
hist_dropin.py and tests/golden/make_hist_golden.py."""
import ctypes as C
import json
import math
import os
import re

import numpy as np

from model_common import _num, _p, bits, same_bits  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "wiggletools_amd", "csrc")
HEADER = os.path.join(CSRC, "wt_hist.h")
WIDTHS = (1, 2, 3, 7, 10, 64, 100)
RANGE_GIVEN, ACCUMULATE = 1, 2


def constants():
    """The WHS_* values of csrc/wt_hist.h: {"BLOCK", "RUNS_PER_LANE", "SHARE", "LDS_WIDTH", "WAVE", "PEEL"}."""
    txt = open(HEADER).read()
    num = lambda k: int(re.search(r"#define WHS_%s (\d+)\b" % k, txt).group(1))      # noqa: E731
    assert re.search(r"#define WHS_BLOCK WCV_BLOCK\b", txt) and re.search(r"#define WHS_SHARE \(WHS_BLOCK \* WHS_RUNS_PER_LANE\)", txt)
    block = int(re.search(r"#define WCV_BLOCK (\d+)", open(os.path.join(CSRC, "wt_cover.h")).read()).group(1))
    c = {k: num(k) for k in ("RUNS_PER_LANE", "LDS_WIDTH", "WAVE", "PEEL")}
    c["BLOCK"] = block
    c["SHARE"] = block * c["RUNS_PER_LANE"]
    return c


class Lists:
    """Run lists as the door takes them: seg (n_seg + 1 offsets), row (n_seg), n_rows, s / f (int32), v (float64)."""

    def __init__(self, seg, row, n_rows, s, f, v):
        self.seg = np.ascontiguousarray(seg, np.int64)
        self.row = np.ascontiguousarray(row, np.int32)
        self.n_rows = int(n_rows)
        self.s, self.f = np.ascontiguousarray(s, np.int32), np.ascontiguousarray(f, np.int32)
        self.v = np.ascontiguousarray(v, np.float64)
        assert len(self.seg) == len(self.row) + 1 and self.seg[-1] == len(self.s) == len(self.f) == len(self.v)

    @classmethod
    def from_rows(cls, rows):
        """One segment per row: rows = [(start, finish, value)]."""
        seg = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])])
        cat = lambda k, t: np.concatenate([np.asarray(r[k], t) for r in rows] + [np.zeros(0, t)])      # noqa: E731
        return cls(seg, np.arange(len(rows)), len(rows), cat(0, np.int32), cat(1, np.int32), cat(2, np.float64))

    def rows(self):
        """[(start, finish, value)] per row, the segments of a row in order."""
        out = []
        for r in range(self.n_rows):
            idx = np.concatenate([np.arange(self.seg[g], self.seg[g + 1]) for g in range(len(self.row)) if self.row[g] == r] + [np.zeros(0, np.int64)]).astype(np.int64)
            out.append((self.s[idx], self.f[idx], self.v[idx]))
        return out

    def seg_rows(self):
        return np.repeat(self.row, np.diff(self.seg)).astype(np.int64)

    def part(self, a, b):
        """The runs [a, b) of the list with the segments cut accordingly."""
        seg = np.clip(self.seg, a, b) - a
        return Lists(seg, self.row, self.n_rows, self.s[a:b], self.f[a:b], self.v[a:b])


def value_range(v):
    """(lo, hi) of the non-NaN values, a zero extreme as +0.0; (nan, nan) when there is none."""
    ok = v[~np.isnan(v)]
    if len(ok) == 0:
        return float("nan"), float("nan")
    return float(ok.min() + 0.0), float(ok.max() + 0.0)


def columns(v, lo, hi, width):
    """The column of every non-NaN value: (int) ((v - lo) * width / (hi - lo)) in double in that order, == width -> width - 1."""
    v = np.asarray(v, np.float64)
    if lo == hi:
        return np.zeros(len(v), np.int64)
    with np.errstate(all="ignore"):
        q = (v - np.float64(lo)) * np.float64(width) / (np.float64(hi) - np.float64(lo))
    return np.where(q < width, np.trunc(np.where(q < width, q, 0.0)), width - 1).astype(np.int64)


def histogram(L, width, given=None, base=None):
    """((lo, hi), (n_rows, width) float64 matrix) by the rule; given: the range of WTAMD_HIST_RANGE_GIVEN; base: the matrix of
    WTAMD_HIST_ACCUMULATE.  Exact integer sums."""
    lo, hi = value_range(L.v) if given is None else (float(given[0]) + 0.0, float(given[1]) + 0.0)
    cnt = np.zeros((L.n_rows, width), np.uint64) if base is None else np.asarray(base, np.float64).astype(np.uint64).reshape(L.n_rows, width)
    ok = ~np.isnan(L.v)
    if ok.any():
        col = columns(L.v[ok], lo, hi, width)
        ln = (L.f[ok].astype(np.int64) - L.s[ok].astype(np.int64)).astype(np.uint64)
        np.add.at(cnt, (L.seg_rows()[ok], col), ln)
    return (lo, hi), cnt.astype(np.float64)


def normalize(m):
    """normalize_histogram: the row sum over the columns in order, then the divisions; an empty row gives NaN."""
    out = np.array(m, np.float64, copy=True)
    for r in range(out.shape[0]):
        total = np.float64(0)
        for x in out[r]:
            total = total + x
        with np.errstate(all="ignore"):
            out[r] = out[r] / total
    return out


def _f(x):
    """printf("%f") of a double."""
    x = float(x)
    if x != x:
        return "-nan" if math.copysign(1.0, x) < 0 else "nan"
    return "%f" % x


def text(rng, m):
    """print_histogram: the centre of every column, found by adding the step again and again, then the rows' cells."""
    lo, hi = np.float64(rng[0]), np.float64(rng[1])
    width = m.shape[1]
    with np.errstate(all="ignore"):
        step = (hi - lo) / np.float64(width)
        pos, lines = lo, []
        for c in range(width):
            lines.append(_f(pos + step / np.float64(2)) + "".join("\t" + _f(m[r, c]) for r in range(m.shape[0])) + "\n")
            pos = pos + step
    return "".join(lines)


def reference_equal(L, width):
    """The condition under which the reference's streaming histogram equals the rule bit for bit: no value outside the interval
    spanned by the stream's first two distinct non-NaN values, and width >= 2 or the second of them higher."""
    stream = np.concatenate([r[2] for r in L.rows()])
    stream = stream[~np.isnan(stream)]
    if len(stream) == 0:
        return False                                    # (the reference does not return)
    a = stream[0]
    other = stream[stream != a]
    if len(other) == 0:
        return True
    b = other[0]
    return bool(stream.min() >= min(a, b) and stream.max() <= max(a, b) and (width >= 2 or b > a))


# ---- fixtures ----
def fixtures():
    return json.load(open(os.path.join(HERE, "golden", "hist_fixtures.json")))["cases"]


def fixture_lists(c):
    return Lists.from_rows([(r["start"], r["finish"], [_num(x) for x in r["value"]]) for r in c["rows"]]), int(c["width"])


def fixture_result(c):
    return (_num(c["range"][0]), _num(c["range"][1])), np.array([[_num(x) for x in row] for row in c["hist"]], np.float64)


def all_fixtures_as_one():
    """Every row of every fixture as a row of one call (one range over all of them): (Lists, rows per fixture).  The segments
    come in reverse order, so seg_row is not the identity."""
    rows = []
    for c in fixtures():
        rows.extend(fixture_lists(c)[0].rows())
    order = list(range(len(rows)))[::-1]
    seg = np.concatenate([[0], np.cumsum([len(rows[r][0]) for r in order])])
    cat = lambda k, t: np.concatenate([np.asarray(rows[r][k], t) for r in order])      # noqa: E731
    return Lists(seg, order, len(rows), cat(0, np.int32), cat(1, np.int32), cat(2, np.float64)), len(rows)


# ---- the emulated passes and the host sweep ----
def emu_lib():
    """tests/emu/libwt_hist_emu.so, built (tests/emu/build.py) and loaded once."""
    from emu import build
    return build.load_unit("hist")


def _call(fn, head, L, width, flags, given, base, dtype=None):
    r2 = np.full(2, -1.0) if given is None else np.array(given, np.float64)
    out = np.full((max(L.n_rows, 1), max(width, 1)), -1.0) if base is None else np.array(base, np.float64, copy=True)
    v = L.v if dtype is None else np.ascontiguousarray(L.v, dtype)
    tail = [] if dtype is None else [C.c_int(1 if v.dtype == np.float64 else 0)]
    rc = fn(*head, C.c_int64(len(L.row)), _p(L.seg), _p(L.row), C.c_int32(L.n_rows), _p(L.s), _p(L.f), _p(v), *tail, C.c_int32(width),
            C.c_uint32(flags), _p(r2), _p(out))
    return rc, r2, out


def emu_door(L, width, order=0, seed=1, flags=0, given=None, base=None, dtype=np.float64):
    """whs_door over the CPU launcher: (rc, range, matrix); the outputs start as -1 (or the inputs)."""
    fn = emu_lib().hist_emu_door
    r2 = np.full(2, -1.0) if given is None else np.array(given, np.float64)
    out = np.full((max(L.n_rows, 1), max(width, 1)), -1.0) if base is None else np.array(base, np.float64, copy=True)
    v = np.ascontiguousarray(L.v, dtype)
    rc = fn(C.c_int(order), C.c_uint64(seed), C.c_int64(len(L.row)), _p(L.seg), _p(L.row), C.c_int32(L.n_rows), _p(L.s), _p(L.f), _p(v),
            C.c_int(1 if v.dtype == np.float64 else 0), C.c_int32(width), C.c_uint32(flags), _p(r2), _p(out), None)
    return rc, r2, out


def host_sweep(L, width, flags=0, given=None, base=None):
    """whs_host: (rc, range, matrix)."""
    return _call(emu_lib().hist_host, [], L, width, flags, given, base)


# ---- seam cases ----
def _runs(rng, n, values, lengths=(1, 2, 3, 5, 40)):
    """n runs, neither sorted nor disjoint, with the given values (cycled)."""
    s = rng.integers(1, 10 ** 6, n).astype(np.int32)
    ln = np.asarray(lengths)[rng.integers(0, len(lengths), n)]
    v = np.resize(np.asarray(values, np.float64), n) if n else np.zeros(0)
    return s, (s + ln).astype(np.int32), v


def edge_values(lo, hi, width):
    """float32 values on and next to every bin edge of [lo, hi] (as doubles)."""
    lo32, hi32 = np.float32(lo), np.float32(hi)
    k = np.arange(width + 1, dtype=np.float64)
    e = (np.float64(lo32) + k * (np.float64(hi32) - np.float64(lo32)) / width).astype(np.float32)
    e[0], e[-1] = lo32, hi32
    allv = np.concatenate([e, np.nextafter(e, np.float32(np.inf)), np.nextafter(e, np.float32(-np.inf))])
    allv = allv[(allv >= lo32) & (allv <= hi32)]
    return np.concatenate([[lo32, hi32], allv]).astype(np.float64)


def seam_cases():
    """{name: (Lists, width)}: every size at which the passes take another path.  All values are exact in float32."""
    c = constants()
    S, W, WV = c["SHARE"], c["LDS_WIDTH"], c["WAVE"]
    rng = np.random.default_rng(20261101)
    out = {}
    k8 = rng.integers(-40, 41, 8 * S) / 8.0
    # rows of S - 1, S, S + 1 and 3 S + 1 runs (so row boundaries fall inside a share), an empty row between two others, an
    # all-NaN row
    sizes = [S - 1, S + 1, 0, 3 * S + 1, WV + 6, S]
    rows = [_runs(rng, n, k8[:max(n, 1)]) for n in sizes]
    rows[4] = (rows[4][0], rows[4][1], np.full(sizes[4], np.nan))
    rows[0][2][::5] = np.nan
    out["rows"] = (Lists.from_rows(rows), 7)
    # chromosome-major: the segments of a row are not adjacent; and track-major with several segments per row
    per = [_runs(rng, n, k8[:max(n, 1)]) for n in (S // 2 + 3, 17, 0, S + 9, 5, S // 2, 0, 3, 2 * S + 1)]
    seg = np.concatenate([[0], np.cumsum([len(p[0]) for p in per])])
    cat = lambda k: np.concatenate([p[k] for p in per])      # noqa: E731
    out["chromosome_major"] = (Lists(seg, [0, 1, 2] * 3, 3, cat(0), cat(1), cat(2)), 10)
    out["track_major"] = (Lists(seg, [0, 0, 0, 1, 1, 1, 3, 3, 3], 4, cat(0), cat(1), cat(2)), 10)
    # both regimes at widths 1, 2, LDS_WIDTH and LDS_WIDTH + 1
    n = S + 3 * WV + 5
    for w in (1, 2, W, W + 1):
        head = [0.0, float(w)]                              # the extremes first: column k holds the values in [k, k + 1)
        mid = float(w // 2) + 0.5 if w > 1 else 0.5
        out["one_column_w%d" % w] = (Lists.from_rows([_runs(rng, n, head + [mid] * (n - 2))]), w)
        out["two_columns_w%d" % w] = (Lists.from_rows([_runs(rng, n, head + [0.25, w - 0.25] * (n // 2))]), w)
        spread = [(i % WV) * (w / float(WV)) + 1.0 / 64 for i in range(n - 2)]
        out["wave_of_columns_w%d" % w] = (Lists.from_rows([_runs(rng, n, head + spread)]), w)
        s, f, v = _runs(rng, 40, head + [mid] * 38)
        s[5:10] = 1
        f[5:10] = 1 + 2 ** 30                               # five runs of 2^30 in one column, and a sixth: past 2^32
        s[11], f[11] = 7, 7 + 2 ** 30
        out["past_2_32_w%d" % w] = (Lists.from_rows([(s, f, v), _runs(rng, 9, [mid])]), w)
    # values on exact bin edges: width 8 over [0, 1] (exact quotients), widths 3, 7, 10 over [0.1, 0.7] (rounded quotients)
    out["edges_w8"] = (Lists.from_rows([_runs(rng, 27, edge_values(0.0, 1.0, 8))]), 8)
    for w in (3, 7, 10):
        ev = edge_values(0.1, 0.7, w)
        out["edges_w%d" % w] = (Lists.from_rows([_runs(rng, len(ev), ev), _runs(rng, len(ev), ev[::-1])]), w)
    # v == hi lands in width - 1; lo == hi
    out["top"] = (Lists.from_rows([_runs(rng, 70, [-3.0, 5.0, 5.0, 5.0])]), 5)
    out["one_value"] = (Lists.from_rows([_runs(rng, S + 1, [2.5]), _runs(rng, 3, [2.5, np.nan])]), 6)
    out["minus_zero"] = (Lists.from_rows([_runs(rng, 9, [-0.0])]), 3)
    out["no_value"] = (Lists.from_rows([_runs(rng, 9, [np.nan]), _runs(rng, 0, [])]), 4)
    for name, (L, w) in out.items():
        assert np.array_equal(L.v.astype(np.float32).astype(np.float64), L.v, equal_nan=True), name
    return out


def refusals():
    """[(name, Lists, width, flags, given, base)]: calls the door refuses with WTAMD_ERR_ARG before it writes anything.  The
    offending run lies in the second workgroup's share."""
    S = constants()["SHARE"]
    rng = np.random.default_rng(20261102)
    n = S + 10

    def lists(**kw):
        s, f, v = _runs(rng, n, rng.integers(0, 9, n) / 8.0)
        L = Lists.from_rows([(s, f, v), _runs(rng, 5, [0.5])])
        for k, x in kw.items():
            getattr(L, k)[S + 5 if k in "sfv" else 1] = x
        return L

    good = lists()
    base = np.zeros((2, 4))
    bad_base = base.copy()
    bad_base[1, 2] = 0.5
    inv = lists()
    inv.s[S + 5], inv.f[S + 5] = 9, 8
    empty = lists()
    empty.f[S + 5] = empty.s[S + 5]
    no_rows = Lists(good.seg, [0, 0], 0, good.s, good.f, good.v)
    return [("width 0", good, 0, 0, None, None), ("no rows", no_rows, 4, 0, None, None),
            ("row == n_rows", lists(row=2), 4, 0, None, None), ("row < 0", lists(row=-1), 4, 0, None, None),
            ("start == finish", empty, 4, 0, None, None), ("start > finish", inv, 4, 0, None, None),
            ("+inf", lists(v=np.inf), 4, 0, None, None), ("-inf", lists(v=-np.inf), 4, 0, None, None),
            ("unknown flag", good, 4, 4, None, None), ("unknown flag beside known ones", good, 4, 8 | RANGE_GIVEN, (0.0, 1.0), None),
            ("accumulate without a range", good, 4, ACCUMULATE, (0.0, 1.0), base),
            ("NaN range", good, 4, RANGE_GIVEN, (np.nan, 1.0), None), ("NaN range above", good, 4, RANGE_GIVEN, (0.0, np.nan), None),
            ("inverted range", good, 4, RANGE_GIVEN, (1.0, 0.0), None),
            ("a value below the range", good, 4, RANGE_GIVEN, (0.125, 1.0), None), ("a value above the range", good, 4, RANGE_GIVEN, (0.0, 0.875), None),
            ("a fraction in the matrix", good, 4, RANGE_GIVEN | ACCUMULATE, (0.0, 1.0), bad_base)]


def check_refusals(door, err):
    """Every refusal returns `err` and leaves the sentinel-filled (or given) outputs as they were.  door(L, width, flags, given,
    base, dtype) -> (rc, range, matrix)."""
    for name, L, w, flags, given, base in refusals():
        for dt in (np.float32, np.float64):
            rc, r2, out = door(L, w, flags, given, base, dt)
            assert rc == err, (name, rc)
            assert same_bits(r2, np.full(2, -1.0) if given is None else np.array(given, np.float64)), (name, r2)
            assert same_bits(out, np.full(out.shape, -1.0) if base is None else base), name


def check_case(door, L, w, what, dtypes=(np.float32, np.float64)):
    """The door against the model; the same values in either width give the same bits."""
    (lo, hi), model = histogram(L, w)
    for dt in dtypes:
        rc, r2, out = door(L, w, 0, None, None, dt)
        assert rc == 0, (what, rc)
        assert same_bits(r2, [lo, hi]), (what, dt, r2, lo, hi)
        assert same_bits(out, model), (what, dt, np.argwhere(bits(out) != bits(model))[:4])
    return (lo, hi), model


def check_split(door, L, w, cuts, what):
    """The list cut at `cuts`: a range per part, their min / max, every part with the range given and accumulated -- the bits
    of the single call."""
    (lo, hi), model = histogram(L, w)
    edges = [0] + sorted(cuts) + [len(L.s)]
    parts = [L.part(a, b) for a, b in zip(edges[:-1], edges[1:])]
    ranges = []
    for p in parts:
        rc, r2, _ = door(p, w, 0, None, None, np.float64)
        assert rc == 0, what
        ranges.append(r2)
    given = (np.nanmin([r[0] for r in ranges]), np.nanmax([r[1] for r in ranges]))
    assert same_bits(given, [lo, hi]), what
    acc = None
    for p in parts:
        rc, r2, acc = door(p, w, RANGE_GIVEN | (ACCUMULATE if acc is not None else 0), given, acc, np.float32)
        assert rc == 0 and same_bits(r2, given), what
    assert same_bits(acc, model), what
