"""Deterministic cases at the edges of the difference-array kernels' exactness proof (wt_delta.h), with plain references.

The proof: a window of N float tracks whose non-zero values have biased exponents emin .. emax is summed in integers and
trusted when N * 2^(emax - emin + 24) <= 2^53, i.e. when emax - emin <= R = 29 - ceil(lg N).  Every case here puts windows
exactly AT that span and exactly one binade past it, with saturated mantissas (2^24 - 1), and lets the deciding exponent
reach the window by every way a value can: a run inside it, a run that spans its origin (the window base), a run across
one window edge, a default value, a track of a later chunk.  No random generator: every value is ldexp(float32(m), e - 150).

The window grid (wt_plan.h, wt_make_windows): a chromosome's windows start at its smallest run start, so every case
starts a run of window 0 at BASE; all other runs lie strictly inside their window.  The tests assert the window width
and the output run count, so a case that is not aligned as meant fails loudly.

References (none goes through the code under test):
  sum       the f64 sum in track order, an absent track adding its default (reference reducers.c:294-307)
  mean      that sum / N, Python's correctly rounded division
  exact     fractions.Fraction -- `Case.sensitive` cases assert that the sequential sum differs from it somewhere
  var ...   the Fraction value of the reference's formulas as wt_delta.h states them, rounded once
"""
import math
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np

from wiggletools_amd.runlists import RunLists

BASE = 1            # first run start of every case: the origin of the window grid
LEAD, TAIL = 5, 7   # a window's runs are [w0 + LEAD, w1 - TAIL) (window 0: [w0, w1 - TAIL))
M_SAT = (1 << 24) - 1
E0 = 90             # default small exponent (2^-60: no f64 range trouble at any span)
VAR_OPS = ("var", "stddev", "cv")


def max_span(n_tracks):
    """R = 29 - ceil(lg N)"""
    return 29 - (n_tracks - 1).bit_length()


def is_pow2(n):
    return n >= 1 and not (n & (n - 1))


def fval(m, e, neg=False):
    """the float m * 2^(e - 150): biased exponent e (1 .. 254) with a 24-bit mantissa, or a denormal (e = 1, m < 2^23)"""
    assert 0 < m < (1 << 24) and 1 <= e <= 254 and (m >= (1 << 23) or e == 1)
    v = np.float32(math.ldexp(float(np.float32(m)), e - 150))
    assert float(v) == math.ldexp(m, e - 150)
    bits = int(v.view(np.uint32))
    assert (bits >> 23) & 0xff == (e if m >= (1 << 23) else 0)
    return np.float32(-v) if neg else v


def window_run(W, k0, k1=None):
    """[start, finish) of a run from window k0's usual start to window k1's usual finish"""
    k1 = k0 if k1 is None else k1
    return BASE + k0 * W + (LEAD if k0 else 0), BASE + (k1 + 1) * W - TAIL


class Case:
    """t: the RunLists; route: "exact" (difference-array kernel, nothing refused), "patched" (few windows refused: their
    values rewritten), "fallback" (many refused: the general kernel redoes the input), "refused" (either of the two),
    "near" (nothing refused, or few and patched), "off" (never on the difference-array path);
    redo: None (not asserted), "none", "some" (windows redone with another unit than the workgroup's guess);
    all_bad: every window must be refused; sensitive: the sequential sum differs from the exact one somewhere;
    sensitive_rn: it also differs from the exact sum correctly rounded, which is what a kernel that wrongly trusted its
    integer sum would return."""

    def __init__(self, name, t, W, n_windows, n_runs, route, ops=("sum", "mean"), sensitive=False, redo=None, all_bad=False, finite=True,
                 sensitive_rn=False):
        self.name, self.t, self.W, self.n_windows, self.n_runs, self.route = name, t, W, n_windows, n_runs, route
        self.ops, self.sensitive, self.redo, self.all_bad, self.finite = tuple(ops), sensitive, redo, all_bad, finite
        self.sensitive_rn = sensitive_rn
        self.N = t.n_tracks
        self._segs = None
        self._exp = {}

    def segments(self):
        if self._segs is None:
            self._segs = segments(self.t)
        return self._segs

    def expected(self, op, strict=0):
        key = (op, strict)
        if key not in self._exp:
            self._exp[key] = reduce_ref(self.segments(), self.N, op, strict)
        return self._exp[key]


def build(N, W, pieces, defaults=None):
    """pieces(i): the runs of track i as (first window, last window, value)"""
    tracks = []
    for i in range(N):
        runs = []
        for k0, k1, v in pieces(i):
            s, f = window_run(W, k0, k1)
            assert not runs or runs[-1][1] <= s
            runs.append((s, f, v))
        tracks.append([runs])
    return RunLists.from_lists(tracks, defaults, dtype=np.float32)


def per_window(n_win, fn):
    """one run per window: fn(k) -> value or None (absent)"""
    return [(k, k, fn(k)) for k in range(n_win) if fn(k) is not None]


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def segments(t):
    """The multiplexer's sweep in plain Python: (start, finish, in play per track, value or default per track) of every
    stretch between two breakpoints where at least one track is in play."""
    assert t.n_chrom == 1
    N = t.n_tracks
    runs = []
    for i in range(N):
        lo, hi = int(t.seg_off[i]), int(t.seg_off[i + 1])
        runs.append([(int(t.start[g]), int(t.finish[g]), float(t.value[g])) for g in range(lo, hi)])
    pts = sorted({p for r in runs for (s, f, _) in r for p in (s, f)})
    dflt = [float(x) for x in t.defaults]
    ptr = [0] * N
    out = []
    for a, b in zip(pts[:-1], pts[1:]):
        ip, xs = [], []
        for i in range(N):
            r = runs[i]
            while ptr[i] < len(r) and r[ptr[i]][1] <= a:
                ptr[i] += 1
            here = ptr[i] < len(r) and r[ptr[i]][0] <= a
            ip.append(here)
            xs.append(r[ptr[i]][2] if here else dflt[i])
        if any(ip):
            out.append((a, b, ip, xs))
    return out


def seq_sum(xs):
    s = 0.0
    for x in xs:
        s += x
    return s


def exact_sum(xs):
    return sum((Fraction(x) for x in xs), Fraction(0))


def _sqrt_fraction(q):
    with localcontext() as ctx:
        ctx.prec = 80
        return (Decimal(q.numerator) / Decimal(q.denominator)).sqrt()


def exact_var_family(op, ip, xs):
    """The reference's formulas over rationals (wt_delta.h:67-78): the mean is over all N tracks; Var squares the tracks in
    play only, StdDev / CV every track (an absent one enters with its default)."""
    N = len(xs)
    F = [Fraction(x) for x in xs]
    mean = sum(F, Fraction(0)) / N
    if op == "var":
        return float(sum(((mean - v) ** 2 for v, here in zip(F, ip) if here), Fraction(0)) / N)
    sd = _sqrt_fraction(sum(((mean - v) ** 2 for v in F), Fraction(0)) / N)
    if op == "stddev":
        return float(sd)
    if mean == 0:
        return float("nan")
    with localcontext() as ctx:
        ctx.prec = 80
        return float(sd / (Decimal(mean.numerator) / Decimal(mean.denominator)))


def reduce_ref(segs, N, op, strict=0):
    """(chrom, start, finish, value) as oracle.reduce returns them"""
    S, F, V = [], [], []
    for a, b, ip, xs in segs:
        if strict and not all(ip):
            continue
        if op == "sum":
            v = seq_sum(xs)
        elif op == "mean":
            v = seq_sum(xs)
            v = v / N if math.isfinite(v) else v
        else:
            v = exact_var_family(op, ip, xs)
        S.append(a); F.append(b); V.append(v)
    return np.zeros(len(S), np.int32), np.array(S, np.int32), np.array(F, np.int32), np.array(V, np.float64)


def sequential_is_exact(case):
    """per emitted stretch: does the sequential f64 sum equal the exact sum?"""
    return [Fraction(seq_sum(xs)) == exact_sum(xs) for (_, _, _, xs) in case.segments()]


def sequential_is_rounded_exact(case):
    """per emitted stretch: does the sequential f64 sum equal the exact sum rounded once (to nearest, ties to even)?"""
    def rn(q):
        return q.numerator / q.denominator      # (int / int: correctly rounded)
    return [seq_sum(xs) == rn(exact_sum(xs)) for (_, _, _, xs) in case.segments()]


# ---------------------------------------------------------------------------
# the cases (R = max_span(N); over = 0: span R, over = 1: span R + 1)
# ---------------------------------------------------------------------------
def _tag(over):
    return "R+1" if over else "R"


def _sensitive(N, over):
    # N - 1 saturated values at span R + 1 reach (1 - 1/N) 2^54 units: past 2^53 for a power of two >= 8 (the issue's observation)
    return bool(over) and is_pow2(N) and N >= 8


def span_edge(N, W, over, n_win=48, ends=None, inf=False, small_track=0, tail2=False, ops=("sum", "mean"), case_no=1):
    """Cases 1, 2, 7, 8.  `small_track` carries the small value (2^24 - 1 at e0) in every window; the others carry 2^24 - 1
    at e0 + span in ONE window and at e0 elsewhere.  ends: "denormal" (e0 = 1 and the small value 2^-149), "top"
    (e0 + R = 254).  inf: one value of the wide window is Inf.
    tail2: the small value sits in the LAST TWO tracks instead.  With the small value first, the sequential sum at R + 1 rounds
    once, a tie, and so does the conversion of the exact integer sum: the same double -- a kernel that wrongly accepted the
    window would differ from the exact rational sum but not from the reference.  With two small values after N - 2 large
    ones (already past 2^53 units for a power of two N >= 8) the sequential sum rounds twice, both ties upwards (the partial
    sums are 3 mod 4 units), and ends 2 units above the exact sum, which is even and a double: `sensitive_rn`."""
    R = max_span(N)
    span = R + over
    e0 = {None: E0, "denormal": 1, "top": 254 - R}[ends]
    assert not (ends == "top" and over)
    small = fval(1, 1) if ends == "denormal" else fval(M_SAT, e0)
    low, big = fval(M_SAT, e0), fval(M_SAT, e0 + span)
    wide = n_win // 2
    inf_track = (N - 1) if small_track != N - 1 else 0
    smalls = (N - 2, N - 1) if tail2 else (small_track,)
    assert not tail2 or (N >= 4 and not inf)

    def pieces(i):
        def v(k):
            if inf and i == inf_track and k == wide:
                return np.float32(np.inf)
            if i in smalls and N > 1:
                return small
            if k == wide:
                return big
            return small if N == 1 else low
        return per_window(n_win, v)

    refused = bool(over) or inf
    route = "exact" if not refused else ("patched" if n_win >= 16 else "fallback")
    if tuple(ops) != ("sum", "mean") and N < 8:
        route = "off"
    name = "case%d-N%d-%s%s%s%s-w%d" % (case_no, N, _tag(over), "-" + ends if ends else "", "-inf" if inf else "",
                                        "-tail2" if tail2 else "-small@%d" % small_track if small_track else "", n_win)
    return Case(name, build(N, W, pieces), W, n_win, n_win, route, ops=ops, sensitive=_sensitive(N, over) and not inf, finite=not inf,
                sensitive_rn=_sensitive(N, over) and tail2)


def through_base(N, W, over, mirror=False, n_win=48):
    """Case 3.  Track 0 is ONE run over all windows: every window but the first meets its value only in the window base.
    mirror: the long run carries the large exponent, the short runs the small one."""
    span = max_span(N) + over
    small, big = fval(M_SAT, E0), fval(M_SAT, E0 + span)
    lng, short = (big, small) if mirror else (small, big)

    def pieces(i):
        return [(0, n_win - 1, lng)] if i == 0 else per_window(n_win, lambda k: short)

    return Case("case3-N%d-%s%s" % (N, _tag(over), "-mirror" if mirror else ""), build(N, W, pieces), W, n_win, 2 * n_win - 1,
                "fallback" if over else "exact", sensitive=_sensitive(N, over) and not mirror, all_bad=bool(over))


def across_edge(N, W, over, mirror=False, n_win=48, ops=("sum", "mean")):
    """Case 4.  Track 0 holds one run that starts in window k and finishes in window k + 1 (the parked path of the launches with
    squares, the long branch of Sum / Mean) and carries one end of the span; every other run -- one per track and window --
    sits at the other end.  (Track 0 has its runs in the other windows too: a window reads the NEXT run of a track that has
    none in it, so a lone run would put its exponent into every window before it.)"""
    span = max_span(N) + over
    small, big = fval(M_SAT, E0), fval(M_SAT, E0 + span)
    crossing, short = (big, small) if mirror else (small, big)
    k = n_win // 2 - 4

    def pieces(i):
        if i:
            return per_window(n_win, lambda kk: short)
        return per_window(k, lambda kk: short) + [(k, k + 1, crossing)] + [(kk, kk, short) for kk in range(k + 2, n_win)]

    name = "case4-N%d-%s%s%s" % (N, _tag(over), "-mirror" if mirror else "", "-squares" if "var" in ops else "")
    return Case(name, build(N, W, pieces), W, n_win, n_win + 1, "patched" if over else "exact", ops=ops,
                sensitive=_sensitive(N, over) and not mirror)


def speculative(N, W, over, falling=False, bridge=False, n_win=48):
    """Case 5.  Windows 0 .. 16 at one exponent, windows 18 .. at another, `up` = R + over binades away.  Every window is narrow
    in itself, so the result must not depend on the unit the workgroup guessed.  Window 17 is empty -- then window 16 reads
    the next run of every track, window 18's, and at R + 1 is refused for it (conservative: route "near") -- or, with
    `bridge`, sits half way between the two exponents: then no window sees more than half the span and nothing is refused."""
    up = max_span(N) + over
    first, later = (E0 + up, E0) if falling else (E0, E0 + up)

    def pieces(i):
        m = M_SAT - 2 * i           # (odd, 24 bits, different per track)
        def v(k):
            if k == 17:
                return fval(m, E0 + up // 2) if bridge else None
            return fval(m, first if k < 17 else later)
        return per_window(n_win, v)

    redo = "some" if (falling or over) else "none"
    return Case("case5-N%d-%s-%s%s" % (N, _tag(over), "falling" if falling else "rising", "-bridge" if bridge else ""), build(N, W, pieces),
                W, n_win, n_win if bridge else n_win - 1, "exact" if (bridge or not over) else "near", redo=redo)


def nonzero_default(N, W, over, kind="pos", n_win=48):
    """Case 6 (the DF flavour).  kind "pos" / "neg": the data sits at e0, the last track is present in window 0 only and its
    default is +-(2^24 - 1) at e0 + span; "smallest": the default is the SMALLEST value, span binades below the data;
    "many": every track but the first is present in window 0 only with the large default (N - 1 large terms: sensitive)."""
    span = max_span(N) + over
    low, high = fval(M_SAT, E0), fval(M_SAT, E0 + span)
    data, dflt = (high, low) if kind == "smallest" else (low, high)
    if kind == "neg":
        dflt = np.float32(-dflt)
    absent = range(1, N) if kind == "many" else (N - 1,)

    def pieces(i):
        return [(0, 0, data)] if i in absent else per_window(n_win, lambda k: data)

    defaults = [float(dflt) if i in absent else 0.0 for i in range(N)]
    return Case("case6-N%d-%s-%s" % (N, _tag(over), kind), build(N, W, pieces, defaults), W, n_win, n_win,
                "fallback" if over else "exact", sensitive=_sensitive(N, over) and kind == "many", all_bad=bool(over))


def chunked(N, W, over, last):
    """Case 7: more tracks than lanes; the deciding (small) value in the last track of the last chunk, or the first of the first."""
    return span_edge(N, W, over, small_track=N - 1 if last else 0, case_no=7)


def squares(N, W, over):
    """Case 8: Var / StdDev / CV"""
    return span_edge(N, W, over, ops=VAR_OPS, case_no=8)


def _specs(device):
    """(builder, arguments) of every case.  device: the track counts the issue sets for the MI355X run."""
    S = []
    for N in ((8, 9, 64, 65, 128) if device else (1, 2, 3, 4, 5, 8, 9, 64, 65, 128, 129)):
        for over in (0, 1):
            S.append((span_edge, dict(N=N, over=over)))
            S.append((span_edge, dict(N=N, over=over, n_win=6)))
    for N in (8, 64, 128):
        for over in (0, 1):
            S.append((span_edge, dict(N=N, over=over, tail2=True)))
    for N in (8, 9):
        S.append((span_edge, dict(N=N, over=0, ends="denormal")))
        S.append((span_edge, dict(N=N, over=0, ends="top")))
        S.append((span_edge, dict(N=N, over=0, ends="top", inf=True)))
    for N in (8, 9, 64):
        for over in (0, 1):
            for mirror in (False, True):
                S.append((through_base, dict(N=N, over=over, mirror=mirror)))
                S.append((across_edge, dict(N=N, over=over, mirror=mirror)))
    for N in (8, 9):
        for over in (0, 1):
            for mirror in (False, True):
                S.append((across_edge, dict(N=N, over=over, mirror=mirror, ops=VAR_OPS)))
            for falling in (False, True):
                for bridge in (False, True):
                    S.append((speculative, dict(N=N, over=over, falling=falling, bridge=bridge)))
            for kind in ("pos", "neg", "smallest", "many"):
                S.append((nonzero_default, dict(N=N, over=over, kind=kind)))
    for N in ((1100,) if device else (150, 128)):
        for over in (0, 1):
            for last in (True, False):
                S.append((chunked, dict(N=N, over=over, last=last)))
    for N in (7, 8, 9, 16):
        for over in (0, 1):
            S.append((squares, dict(N=N, over=over)))
    return S


def _name(fn, kw):
    parts = [fn.__name__] + ["%s_%s" % (k, "squares" if k == "ops" else kw[k]) for k in sorted(kw)]
    return "-".join(parts)


def specs(device=False, only=None):
    """[(id, builder, arguments)]; only: keep the builders named"""
    return [(_name(fn, kw), fn, kw) for fn, kw in _specs(device) if only is None or fn.__name__ in only]
