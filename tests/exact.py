"""References that are better than the f64 run-by-run update the integrators are usually compared with.

The reference's own update (tests/test_integrator_moments.py::_sequential) loses (mean / deviation)^2 of its digits in
T = S L (v - mean)^2: 7e-15 at mean/dev = 1, 2.4e-7 at 1e6, 0.6 at 1e9 (2e4 runs).  A kernel that claims to do better can
only be held to that claim by something exact:

  moments_exact / pearson_exact   fractions.Fraction up to FRACTION_MAX runs (every double is a rational), above that a corrected
                                  two-pass sum in np.longdouble (64-bit mantissa; agrees with Fraction to ~1e-16 on every
                                  conditioning class tried, tests/test_side_kernels.py::test_long_double_against_fraction)
  exact_by_construction           run lists whose every partial sum of L * v is a multiple of 1/8 below 2^53: ANY f64
                                  summation order gives the same bits, so one missing, doubled or misplaced run shows
  seq_moments / seq_pearson       the run-by-run f64 updates, compiled (tests/seq_moments.c): their error against the
                                  exact values is what the device's bound is derived from
"""
import ctypes as C
import os
import subprocess
import tempfile
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FRACTION_MAX = 100_000


def long_double_ok():
    """np.longdouble carries at least the x87 64-bit mantissa (it is a plain double on some platforms)"""
    return np.finfo(np.longdouble).nmant >= 63


def _first_extreme(v, kind):
    """The reference's MaxPop / MinPop (statistics.c:176,206): strict > / <, so the FIRST run that reaches the extreme stays --
    which decides the sign of a zero result.  NaN when there is no run."""
    if len(v) == 0:
        return float("nan")
    e = v.max() if kind == "max" else v.min()
    return float(v[np.flatnonzero(v == e)[0]])          # (-0.0 == 0.0: the first of either)


def _split(start, finish, value):
    value = np.asarray(value, np.float64)
    ok = ~np.isnan(value)
    L = (np.asarray(finish, np.int64) - np.asarray(start, np.int64))[ok]
    return L, value[ok]


def _two_pass_ld(L, cols):
    """Corrected two-pass sums in long double.  cols: list of f64 arrays.  Returns (span, [sums], {(i, j): T_ij})."""
    assert long_double_ok()
    ld = np.longdouble
    Ll = L.astype(ld)
    span = Ll.sum()
    sums = [(Ll * c.astype(ld)).sum() for c in cols]
    dev = [c.astype(ld) - s / span for c, s in zip(cols, sums)]
    corr = [(Ll * d).sum() for d in dev]                # (what the rounded mean left over: the correction term)
    T = {}
    for i in range(len(cols)):
        for j in range(i, len(cols)):
            T[(i, j)] = (Ll * dev[i] * dev[j]).sum() - corr[i] * corr[j] / span
    return span, sums, T


def _fraction(L, cols):
    Lf = [int(x) for x in L]
    span = sum(Lf)
    F = [[Fraction(x) for x in c.tolist()] for c in cols]
    sums = [sum(l * x for l, x in zip(Lf, c)) for c in F]
    T = {}
    for i in range(len(cols)):
        for j in range(i, len(cols)):
            s2 = sum(l * x * y for l, x, y in zip(Lf, F[i], F[j]))
            T[(i, j)] = s2 - sums[i] * sums[j] / span if span else Fraction(0)
    return span, sums, T


def moments_exact(start, finish, value, method=None):
    """(sum, span, T, min, max) over the non-NaN runs, each the f64 nearest the exact value (Fraction) or within ~1e-19
    relative of it before the final rounding (long double).  method: None (by size), "fraction", "longdouble"."""
    L, v = _split(start, finish, value)
    mn, mx = _first_extreme(v, "min"), _first_extreme(v, "max")
    if len(v) == 0:
        return 0.0, 0.0, 0.0, mn, mx
    if method is None:
        method = "fraction" if len(v) <= FRACTION_MAX else "longdouble"
    span, sums, T = (_fraction if method == "fraction" else _two_pass_ld)(L, [v])
    return float(sums[0]), float(span), float(T[(0, 0)]), mn, mx


def pearson_exact(start, finish, values, inplay, defaults, method=None):
    """{n, Sx, Sy, Txx, Txy, Tyy} of a 2-track Multiplexer tile (values[R, 2], inplay[R, 2]; a track that is not in play
    contributes its default -- statistics.c:414-465 reads the Multiplexer's filled-in values) and the correlation
    Txy / sqrt(Txx Tyy) computed from the exact moments."""
    d = np.asarray(defaults, np.float64)
    x = np.where(np.asarray(inplay)[:, 0] != 0, np.asarray(values, np.float64)[:, 0], d[0])
    y = np.where(np.asarray(inplay)[:, 1] != 0, np.asarray(values, np.float64)[:, 1], d[1])
    L = np.asarray(finish, np.int64) - np.asarray(start, np.int64)
    if len(L) == 0:
        return np.zeros(6), float("nan")
    if method is None:
        method = "fraction" if len(L) <= FRACTION_MAX else "longdouble"
    span, sums, T = (_fraction if method == "fraction" else _two_pass_ld)(L, [x, y])
    m = np.array([float(span), float(sums[0]), float(sums[1]), float(T[(0, 0)]), float(T[(0, 1)]), float(T[(1, 1)])])
    den = T[(0, 0)] * T[(1, 1)]
    if method == "fraction":
        r = float(T[(0, 1)]) / float(np.sqrt(np.longdouble(float(T[(0, 0)])) * np.longdouble(float(T[(1, 1)])))) if den else float("nan")
    else:
        r = float(T[(0, 1)] / np.sqrt(den)) if den else float("nan")
    return m, r


def exact_by_construction(rng, n, max_len=8, levels=800, signed=False, nan_prob=0.0, gap_prob=0.1):
    """n sorted runs with lengths 1 .. max_len and values k / 8, |k| < levels: every L * v is a multiple of 1/8 and
    n * max_len * levels / 8 must stay below 2^50, so every partial sum in every order is exact in f64.
    Returns (start, finish, value, eighths): eighths = S L k over the non-NaN runs as a Python int (sum = eighths / 8).
    The first and the last run are never NaN and never 0, so a kernel that drops either is caught."""
    assert n * max_len * levels < 2 ** 53
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0), 0
    L = rng.integers(1, max_len + 1, n).astype(np.int64)
    gap = (rng.random(n) < gap_prob) * rng.integers(1, 5, n)
    start = 1 + np.cumsum(gap + np.concatenate([[0], L[:-1]]))
    assert n == 0 or start[-1] + max_len < 2 ** 31
    k = rng.integers(-(levels - 1) if signed else 0, levels, n)
    if n:
        k[0] = k[0] if k[0] else 3
        k[-1] = k[-1] if k[-1] else 5
    v = k / 8.0
    nan = rng.random(n) < nan_prob
    if n:
        nan[0] = nan[-1] = False
    v[nan] = np.nan
    eighths = int((L * k)[~nan].sum())
    return start.astype(np.int32), (start + L).astype(np.int32), v, eighths


def conditioned(seed, n, mean, dev, max_len=49):
    """The issue's conditioning classes: contiguous runs of length 1 .. max_len, values mean + dev * N(0, 1)."""
    rng = np.random.default_rng(seed)
    L = rng.integers(1, max_len + 1, n).astype(np.int64)
    finish = 1 + np.cumsum(L)
    assert finish[-1] < 2 ** 31
    return (finish - L).astype(np.int32), finish.astype(np.int32), mean + dev * rng.standard_normal(n)


# ---- the run-by-run f64 updates, compiled ----
_seq = None


def _seq_lib():
    global _seq
    if _seq is None:
        so = os.path.join(tempfile.mkdtemp(prefix="wt_seq_"), "libseq_moments.so")
        subprocess.check_call(["gcc", "-O1", "-std=c99", "-ffp-contract=off", "-fPIC", "-shared", "-Wall",
                               os.path.join(HERE, "seq_moments.c"), "-o", so])
        _seq = C.CDLL(so)
        _seq.seq_moments.restype = None
        _seq.seq_moments.argtypes = [C.c_int64] + [C.c_void_p] * 4
        _seq.seq_pearson.restype = None
        _seq.seq_pearson.argtypes = [C.c_int64] + [C.c_void_p] * 5
    return _seq


def seq_moments(start, finish, value):
    """test_integrator_moments._sequential, compiled: (T, total, count, min, max)"""
    s, f = np.ascontiguousarray(start, np.int32), np.ascontiguousarray(finish, np.int32)
    v, out = np.ascontiguousarray(value, np.float64), np.zeros(5)
    _seq_lib().seq_moments(len(s), s.ctypes.data, f.ctypes.data, v.ctypes.data, out.ctypes.data)
    return tuple(out.tolist())


def seq_pearson(start, finish, values, inplay, defaults):
    """{n, Sx, Sy, Txx, Txy, Tyy} by the reference's run-by-run update over the filled-in tile"""
    d = np.asarray(defaults, np.float64)
    x = np.ascontiguousarray(np.where(np.asarray(inplay)[:, 0] != 0, np.asarray(values, np.float64)[:, 0], d[0]))
    y = np.ascontiguousarray(np.where(np.asarray(inplay)[:, 1] != 0, np.asarray(values, np.float64)[:, 1], d[1]))
    s, f, out = np.ascontiguousarray(start, np.int32), np.ascontiguousarray(finish, np.int32), np.zeros(6)
    _seq_lib().seq_pearson(len(s), s.ctypes.data, f.ctypes.data, x.ctypes.data, y.ctypes.data, out.ctypes.data)
    return out


def rel_err(got, exact):
    """|got - exact| / |exact| -- relative to the exact value and to nothing else (no max(1, ...): a variance of 1e-12 is held
    as tightly as one of 1e12); 0 where both are the same number, inf where exact is 0 and got is not."""
    if got == exact or (got != got and exact != exact):
        return 0.0
    if exact == 0 or got != got or exact != exact:
        return float("inf")
    return abs(got - exact) / abs(exact)


def same_bits(a, b):
    """-0.0 is not 0.0; the sign / payload of a NaN is not compared"""
    if a != a or b != b:
        return a != a and b != b
    return a == b and np.signbit(a) == np.signbit(b)
