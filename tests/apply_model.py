"""NumPy / Fraction model of the per-region statistics (csrc/wt_apply.h, wtamd_runs_apply: the reference's `apply`,
src/apply.c) and the helpers the apply tests share.

Region [rs, rf) of one segment of a sorted, disjoint dataset: lo = the first run with finish > rs, hi = the first with
start >= rf, the pieces are [max(s, rs), min(f, rf)) of the runs in [lo, hi).  With L the piece lengths and v the values
widened to f64 the six outputs are
    m[0] = S L v    m[1] = S L    m[2] = T = S L (v - m[0]/m[1])^2    m[3] = min    m[4] = max    over the pieces that are not NaN,
    m[5] = covered = S L over all pieces.
Fill-in (strict=False) with a default that is not NaN: the (rf - rs) - covered uncovered base pairs are one more piece with
the default as its value, after the data.  m[0..4] come from exact.moments_exact (rational arithmetic), so a kernel is held
to the exact value: span, covered, min and max bit for bit, the sum bit for bit where the case is exact by construction
(values k / 8) and within sum_bound elsewhere, T within T_bound."""
import ctypes as C
import os
import re

import numpy as np

import exact
from model_common import _p  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "wiggletools_amd", "csrc")

OK, ERR_ARG = 0, 1
STRICT = 1
STATS = ["AUC", "meanI", "varI", "stddevI", "CVI", "maxI", "minI"]      # WTAMD_APPLY_*
DEFAULTS = (0.0, 1.5, float("nan"))


def constants():
    """The WAP_* values of csrc/wt_apply.h: {"SMALL", "CHUNK", "WINDOW", "TILE"}."""
    txt = {n: open(os.path.join(CSRC, n)).read() for n in ("wt_apply.h", "wt_region.h", "wt_cover.h")}
    num = lambda f, name: int(re.search(r"#define %s (\d+)" % name, txt[f]).group(1))      # noqa: E731
    assert re.search(r"#define WAP_WINDOW WRG_WINDOW\b", txt["wt_apply.h"]) and re.search(r"#define WAP_BLOCK WCV_BLOCK\b", txt["wt_apply.h"])
    return {"SMALL": num("wt_apply.h", "WAP_SMALL"), "CHUNK": num("wt_apply.h", "WAP_CHUNK"), "WINDOW": num("wt_region.h", "WRG_WINDOW"),
            "TILE": num("wt_cover.h", "WCV_BLOCK") * num("wt_apply.h", "WAP_PER_LANE")}


def pieces(s, f, v, rs, rf):
    """The run pieces of one segment (s, f, v) under [rs, rf): (start, finish, value as f64)."""
    s, f = np.asarray(s, np.int64), np.asarray(f, np.int64)
    lo = int(np.searchsorted(f, rs, side="right"))
    hi = max(int(np.searchsorted(s, rf, side="left")), lo)
    return np.maximum(s[lo:hi], rs), np.minimum(f[lo:hi], rf), np.asarray(v[lo:hi]).astype(np.float64)


def with_fill(ps, pf, pv, rs, rf, default, strict):
    """The pieces the statistics see: in fill-in mode one more piece of the uncovered length, after the data."""
    u = int(rf) - int(rs) - int((pf - ps).sum())
    if strict or default != default or u <= 0:
        return ps, pf, pv
    return np.concatenate([ps, [0]]), np.concatenate([pf, [u]]), np.concatenate([pv, [default]])


def region_moments(s, f, v, rs, rf, default=0.0, strict=True):
    ps, pf, pv = pieces(s, f, v, rs, rf)
    cov = float((pf - ps).sum())
    return np.array(exact.moments_exact(*with_fill(ps, pf, pv, rs, rf, default, strict)) + (cov,))


def finish(m6, stat):
    """wtamd_apply_finish: the reference's closing arithmetic in its own order (statistics.c:66-67,259,288-289,312-314)."""
    stat = STATS.index(stat) if isinstance(stat, str) else int(stat)
    with np.errstate(all="ignore"):
        m = [np.float64(x) for x in m6]
        if stat == 0:
            return float(m[0])
        if stat == 1:
            return float(m[0] / m[1]) if m[1] > 0 else float("nan")
        if stat == 5:
            return float(m[4])
        if stat == 6:
            return float(m[3])
        res = m[2] / (m[1] - 1)
        if stat >= 3:
            res = np.sqrt(res)
        if stat == 4:
            res = res / (m[0] / m[1])
        return float(res)


def T_bound(ps, pf, pv, t_exact):
    """What the run-by-run f64 update of the reference loses on these pieces, times four, and never below 1e-9: the bound
    tests/test_side_kernels.py holds the integrators to."""
    ok = ~np.isnan(pv)
    seq = exact.seq_moments(ps[ok], pf[ok], pv[ok])[0]
    return max(4 * exact.rel_err(seq, t_exact), 1e-9)


def sum_bound(ps, pf, pv):
    """|sum - exact| a pivoted sum of these pieces may show: at most len + 4 roundings, each of a quantity no larger than
    S L (|v| + |K|), |K| <= max |v|."""
    ok = ~np.isnan(pv)
    if not ok.any():
        return 0.0
    L, a = (pf - ps)[ok].astype(np.float64), np.abs(pv[ok])
    return 2.0 ** -52 * (int(ok.sum()) + 4) * float((L * (a + a.max())).sum())


class Case:
    """data: per segment (start, finish, value); regions: per segment (start, finish).  exact_sum: every value is k / 8."""

    def __init__(self, data, regions, exact_sum=True):
        assert len(data) == len(regions)
        self.data, self.regions, self.exact_sum = data, regions, exact_sum
        self.seg = np.concatenate([[0], np.cumsum([len(d[0]) for d in data])]).astype(np.int64)
        self.rseg = np.concatenate([[0], np.cumsum([len(r[0]) for r in regions])]).astype(np.int64)
        cat = lambda parts, dt: np.concatenate([np.asarray(p) for p in parts] + [np.zeros(0)]).astype(dt)      # noqa: E731
        self.s, self.f = cat([d[0] for d in data], np.int32), cat([d[1] for d in data], np.int32)
        self.v = cat([d[2] for d in data], np.float64)
        assert np.array_equal(self.v.astype(np.float32).astype(np.float64), self.v, equal_nan=True)        # the same values in f32
        self.rs, self.rf = cat([r[0] for r in regions], np.int32), cat([r[1] for r in regions], np.int32)
        self._exp = {}

    def values(self, dt):
        return self.v.astype(dt)

    def expected(self, default, strict):
        """[(m6, T bound, sum bound)] per region, computed once per (default, mode)."""
        key = "strict" if strict or default != default else repr(float(default))
        if key not in self._exp:
            rows = []
            for (s, f, v), (rs_, rf_) in zip(self.data, self.regions):
                for a, b in zip(rs_, rf_):
                    ps, pf, pv = pieces(s, f, v, int(a), int(b))
                    cov = float((pf - ps).sum())
                    qs, qf, qv = with_fill(ps, pf, pv, int(a), int(b), default, key == "strict")
                    m = np.array(exact.moments_exact(qs, qf, qv) + (cov,))
                    rows.append((m, T_bound(qs, qf, qv, m[2]), sum_bound(qs, qf, qv)))
            self._exp[key] = rows
        return self._exp[key]

    def subset(self, idx):
        """The case with only the regions idx (positions in the flat region list)."""
        idx = np.asarray(idx)
        regs = []
        for g in range(len(self.regions)):
            k = idx[(idx >= self.rseg[g]) & (idx < self.rseg[g + 1])] - self.rseg[g]
            regs.append((np.asarray(self.regions[g][0])[k], np.asarray(self.regions[g][1])[k]))
        return Case(self.data, regs, self.exact_sum)


def check(case, got, default, strict, what=""):
    """got: (n, 6) from a kernel, the emulator or the host sweep, against the model."""
    exp = case.expected(default, strict)
    assert got.shape == (len(exp), 6), (what, got.shape, len(exp))
    for i, (m, tb, sb) in enumerate(exp):
        g = got[i]
        w = (what, i, g.tolist(), m.tolist())
        assert g[1] == m[1] and g[5] == m[5], w
        assert exact.same_bits(g[3], m[3]) and exact.same_bits(g[4], m[4]), w
        if case.exact_sum:
            assert g[0] == m[0], w                 # (== : the sign of a zero sum is not part of the claim)
        else:
            assert abs(g[0] - m[0]) <= sb, w
        assert exact.rel_err(g[2], m[2]) <= tb, w + (tb,)


def same_rows(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64) | (np.isnan(a) * np.uint64(0xffffffffffffffff)),
                                                 b.view(np.uint64) | (np.isnan(b) * np.uint64(0xffffffffffffffff)))


# ---- case builders ----
def dataset(rng, n, exact_sum=True, nan_prob=0.0, gap_prob=0.15, first=1):
    """n sorted disjoint runs of length 1 .. 8, some touching, some apart; values k / 8 (|k| < 80) or, with exact_sum=False,
    float32 normals around 100.  NaN runs with probability nan_prob."""
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0)
    s, f, v, _ = exact.exact_by_construction(rng, n, max_len=8, levels=80, signed=True, nan_prob=nan_prob, gap_prob=gap_prob)
    if not exact_sum:
        w = (100.0 + rng.standard_normal(n)).astype(np.float32).astype(np.float64)
        v = np.where(np.isnan(v), np.nan, w)
    return (s + (first - 1)).astype(np.int32), (f + (first - 1)).astype(np.int32), v


def over_runs(d, a, b, clip=True):
    """A region over the runs a .. b - 1 of dataset d, ending inside the first and the last when it can."""
    s, f = d[0], d[1]
    rs = int(s[a]) + (1 if clip and f[a] - s[a] > 1 else 0)
    rf = int(f[b - 1]) - (1 if clip and f[b - 1] - s[b - 1] > 1 and (b - 1 > a or f[a] - rs > 1) else 0)
    return rs, rf


def random_regions(rng, d, n, max_runs):
    """n regions sorted by start over dataset d: each from somewhere in or next to a run to 1 .. max_runs runs further;
    overlapping, nested and repeated ones among them."""
    s, f = d[0].astype(np.int64), d[1].astype(np.int64)
    a = np.sort(rng.integers(0, len(s), n))
    b = np.minimum(a + rng.integers(1, max_runs + 1, n), len(s))
    rs = s[a] + rng.integers(-2, 3, n)
    rf = f[b - 1] + rng.integers(-2, 3, n)
    rs = np.maximum(rs, 0)
    rf = np.maximum(rf, rs + 1)
    rep = np.nonzero(rng.random(n) < 0.05)[0]
    rep = rep[rep > 0]
    rs[rep], rf[rep] = rs[rep - 1], rf[rep - 1]
    o = np.argsort(rs, kind="stable")
    return rs[o].astype(np.int32), rf[o].astype(np.int32)


def seam_cases():
    """{name: Case} at the sizes where the passes change lane, chunk, tile or search path (also run on the device)."""
    c = constants()
    S, CH, W, T = c["SMALL"], c["CHUNK"], c["WINDOW"], c["TILE"]
    rng = np.random.default_rng(12)
    out = {}
    empty_d = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    empty_r = (np.zeros(0, np.int32), np.zeros(0, np.int32))
    reg = lambda pairs: (np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32))      # noqa: E731
    # n runs under one region, its first and its last run clipped; exact values and float ones, NaN runs among them
    for n in (S - 1, S, S + 1, CH - 1, CH, CH + 1, 3 * CH + 5):
        for ex in (True, False):
            d = dataset(rng, n + 20, ex, nan_prob=0.1)
            r = over_runs(d, 7, 7 + n)
            assert len(pieces(d[0], d[1], d[2], *r)[0]) == n
            # the same region three times, one nested inside it, and a small one behind it
            out["runs%d%s" % (n, "" if ex else "_float")] = Case([d], [reg([r, r, r, over_runs(d, 9, 9 + n // 2), over_runs(d, n + 10, n + 15)])], ex)
    # T - 1 .. 3T + 5 regions, most in the lane regime, some in the chunk regime in every tile
    for n in (T - 1, T, T + 1, 3 * T + 5):
        d = dataset(rng, 2 * n, True, nan_prob=0.05)
        rs, rf = random_regions(rng, d, n, 12)
        big = rng.choice(n, 9, replace=False)
        for k in big:
            a = int(np.searchsorted(d[1], rs[k], side="right"))
            b = min(a + S + 1 + int(rng.integers(0, 2 * S)), len(d[0]))
            rf[k] = max(int(d[1][b - 1]) - 1, int(rs[k]) + 1)
        out["regions%d" % n] = Case([d], [(rs, rf)], True)
    # one tile whose window is exactly W, and W + 1, dataset runs: staged in LDS, and searched in global memory
    for w in (W, W + 1):
        d = dataset(rng, w + 30, True, nan_prob=0.02)
        first, last = over_runs(d, 11, 14), over_runs(d, 11 + w - 5, 11 + w)
        a = np.sort(np.concatenate([[12], rng.integers(12, 11 + w - 6, 200)]))         # (the 12: a chunk-regime region in the window)
        b = np.minimum(a + rng.integers(1, 7, len(a)), 11 + w - 1)
        b[0] = 12 + S + 3
        rs = np.concatenate([[first[0]], d[0][a], [last[0]]])
        rf = np.concatenate([[first[1]], d[1][b - 1], [last[1]]])
        assert (np.diff(rs) >= 0).all() and rf.max() == last[1] and (rf > rs).all()
        out["window%d" % w] = Case([d], [(rs.astype(np.int32), rf.astype(np.int32))], True)
    # several segments inside one tile: an empty dataset, no regions, neither, and ordinary ones
    ds = [dataset(rng, k, True, nan_prob=0.1) for k in (40, 7, 90, 3)]
    out["segments"] = Case([ds[0], empty_d, ds[1], empty_d, ds[2], empty_d, ds[3]],
                           [random_regions(rng, ds[0], 20, 9), reg([(3, 9), (5, 50)]), empty_r, empty_r, random_regions(rng, ds[2], 50, 40),
                            empty_r, random_regions(rng, ds[3], 4, 3)])
    many_d = [dataset(rng, int(rng.integers(1, 200)), True) if k % 5 else empty_d for k in range(40)]
    out["segments_many"] = Case(many_d, [random_regions(rng, d, int(rng.integers(1, 60)), 50) if (k % 3 and len(d[0])) else
                                         (reg([(1, 4), (2, 3)]) if k % 3 else empty_r) for k, d in enumerate(many_d)])
    # edges, spelled out: runs [10,20) = 1, [20,25) = NaN, [30,40) = -0.0, [40,41) = 0.0, [50,60) = 2.5
    d = (np.array([10, 20, 30, 40, 50], np.int32), np.array([20, 25, 40, 41, 60], np.int32), np.array([1.0, np.nan, -0.0, 0.0, 2.5]))
    out["edges"] = Case([d], [reg([(1, 5), (1, 10), (1, 11), (5, 70), (10, 20), (12, 18), (12, 18), (19, 21), (20, 25), (20, 30), (25, 30), (26, 29),
                                   (30, 41), (39, 52), (40, 41), (59, 60), (60, 61), (60, 900), (70, 80)])])
    return out


def mid_size():
    """40 000 runs, 5 000 random regions, and one region over all of it."""
    rng = np.random.default_rng(21)
    d = dataset(rng, 40000, False, nan_prob=0.01)
    rs, rf = random_regions(rng, d, 5000, 60)
    rs = np.concatenate([[0], rs]).astype(np.int32)
    rf = np.concatenate([[int(d[1][-1]) + 5], rf]).astype(np.int32)
    return Case([d], [(rs, rf)], False)


# ---- the passes of csrc/wt_apply.h on the CPU (tests/apply_emu.cpp) ----
def emu_lib():
    """tests/emu/libwt_apply_emu.so, built (tests/emu/build.py) and loaded once."""
    from emu import build
    return build.load_unit("apply")


def emu_apply(seg, s, f, v, rseg, rs, rf, default=0.0, strict=True, order=0, seed=0, flags=None):
    """Returns (rc, (n, 6)); the output starts out filled with -1 and a refused call leaves it so."""
    seg, rseg = np.ascontiguousarray(seg, np.int64), np.ascontiguousarray(rseg, np.int64)
    s, f = np.ascontiguousarray(s, np.int32), np.ascontiguousarray(f, np.int32)
    rs, rf = np.ascontiguousarray(rs, np.int32), np.ascontiguousarray(rf, np.int32)
    v = np.ascontiguousarray(v)
    assert v.dtype in (np.float32, np.float64)
    out = np.full((max(len(rs), 1), 6), -1.0)
    fl = (STRICT if strict else 0) if flags is None else flags
    rc = emu_lib().apply_emu(C.c_int(order), C.c_uint64(seed), C.c_int64(len(seg) - 1), _p(seg), _p(s), _p(f), _p(v), C.c_int(int(v.dtype == np.float64)),
                             _p(rseg), _p(rs), _p(rf), C.c_double(default), C.c_uint32(fl), _p(out))
    return rc, out[:len(rs)]


def emu_case(case, default=0.0, strict=True, dt=np.float64, **kw):
    return emu_apply(case.seg, case.s, case.f, case.values(dt), case.rseg, case.rs, case.rf, default, strict, **kw)


def host_sweep(case, default=0.0, strict=True):
    """The host sweep of csrc/wt_apply.h, segment pair by segment pair."""
    out = np.full((max(len(case.rs), 1), 6), -1.0)
    for g in range(len(case.seg) - 1):
        a, b, ra, rb = int(case.seg[g]), int(case.seg[g + 1]), int(case.rseg[g]), int(case.rseg[g + 1])
        s, f, v = (np.ascontiguousarray(x[a:b]) for x in (case.s, case.f, case.v))
        rs, rf = np.ascontiguousarray(case.rs[ra:rb]), np.ascontiguousarray(case.rf[ra:rb])
        part = np.full((max(rb - ra, 1), 6), -1.0)
        rc = emu_lib().apply_host(C.c_int64(b - a), _p(s), _p(f), _p(v), C.c_int64(rb - ra), _p(rs), _p(rf), C.c_double(default),
                                  C.c_uint32(STRICT if strict else 0), _p(part))
        if rc != 0:
            return rc, out[:0]
        out[ra:rb] = part[:rb - ra]
    return 0, out[:len(case.rs)]


# ---- the recordings of the compiled reference (tests/golden/apply_fixtures.json) ----
def load_fixtures():
    import json
    return json.load(open(os.path.join(HERE, "golden", "apply_fixtures.json")))["cases"]


def _num(x):
    return float("nan") if x is None else float(x)


def fixture_case(c):
    """A recorded case as (Case over every chromosome name of the case -- a chromosome one side lacks is an empty segment --,
    default).  The regions come out in the order the reference served them: chromosome by chromosome."""
    n = len(c["chrom_names"])
    empty_d, empty_r = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0)), (np.zeros(0, np.int32), np.zeros(0, np.int32))
    data, regs = [empty_d] * n, [empty_r] * n
    d, r = c["data"], c["regions"]
    val = np.array([_num(x) for x in d["value"]], np.float64)
    for k, g in enumerate(d["chroms"]):
        a, b = d["seg_off"][k], d["seg_off"][k + 1]
        data[g] = (np.array(d["start"][a:b], np.int32), np.array(d["finish"][a:b], np.int32), val[a:b])
    for k, g in enumerate(r["chroms"]):
        a, b = r["seg_off"][k], r["seg_off"][k + 1]
        regs[g] = (np.array(r["start"][a:b], np.int32), np.array(r["finish"][a:b], np.int32))
    return Case(data, regs, True), _num(c["default"])


def recorded(rec, stat):
    return [float(x) if isinstance(x, str) else _num(x) for x in rec[stat]] if stat in rec else None


def reference_stops(case):
    """Where the reference's dataset ends for every region: ApplyMultiplexer buffers regions in groups (apply.c:196-217:
    a region joins while it starts at most 10 bp behind the largest finish so far, on the same chromosome) and seeks the
    dataset to [first start, LAST region's finish) of the group (apply.c:311) -- so a region that reaches past the finish of
    the last region of its group (one nested in it follows it) loses the data beyond.  Returns the stop per region."""
    stops = np.zeros(len(case.rs), np.int64)
    for g in range(len(case.rseg) - 1):
        a, b = int(case.rseg[g]), int(case.rseg[g + 1])
        i = a
        while i < b:
            j, last = i + 1, int(case.rf[i])
            while j < b and int(case.rs[j]) <= last + 10:
                last = max(last, int(case.rf[j]))
                j += 1
            stops[i:j] = int(case.rf[j - 1])
            i = j
    return stops


def all_fixtures_in_one(cases):
    """Every recorded case as further segments of ONE call: (Case, [default per case], [region range per case])."""
    data, regs, spans = [], [], []
    n = 0
    for c in cases:
        k, _ = fixture_case(c)
        data += k.data
        regs += k.regions
        spans.append((n, n + len(k.rs)))
        n += len(k.rs)
    return Case(data, regs, True), spans
