"""Constructed columns for the t-test's tail (a helper, not a test module: tests/test_ttest_tail_plane.py).

Every position is one 1-bp run in every track, so one track set yields P chosen (t, nu) pairs.  Per position: amplitudes
A1, A2 in {1/8 .. 63/8} and a shift d, a multiple of 1/8; set 0 is +-A1 + d/2 alternating (the last value d/2 when n1 is odd),
set 1 is +-A2 - d/2.  Every value is exact in float32 and every sum and sum of squares exact in f64 for n <= 4200, so the
device, the emulator and the oracle hold the same (t, nu) bit for bit: only the tail differs.

  benign     d log-uniform, capped at 60 min over the sets of A sqrt((n - odd) / n): var * 1024 >= meanSq in both sets
             (wt_ttest_stat's `risk` stays clear: var = A^2 (n - odd) / n, meanSq = var + d^2 / 4, so 1023 var >= d^2 / 4
             needs d <= 63.9 A sqrt((n - odd) / n)); every 7th column d = 0 (t = 0, p = 1)
  separated  70 max(A1, A2) <= d <= 1000: `risk` is set, the window goes to wt_patch_kernel or the launch is redone;
             followed by the edge columns: both sets constant (NaN, setComparisons.c:98), one set constant (nu = n_other - 1)
"""
import math

import numpy as np

from wiggletools_amd.runlists import RunLists

SIZES = [(2, 2), (2, 3), (3, 3), (3, 4), (3, 9), (4, 4), (8, 8), (16, 17), (17, 17), (50, 50), (33, 300), (450, 450), (1001, 1001),
         (1002, 1002), (2100, 2100)]
# a set of fewer than 3 tracks is refused by the product as by the reference (setComparisons.c:123-128): 2 v 2, 2 v 3 and
# 1 v 9 (nu = 0 / 0) reach the oracle, the emulator and the host-compiled tail only; nu < 2 cannot occur on the device
DEVICE_SIZES = [s for s in SIZES if min(s) >= 3]
DELTA_SIZES = [s for s in DEVICE_SIZES if s[0] + s[1] >= 8]     # float tracks: the difference-array kernel (wt_plan.h)
P_BENIGN = 200
P_SEPARATED = 48
N_EDGE = 8
WINDOW = 2048


def _harmonic(n1, n2):
    return 1.0 / (1.0 / n1 + 1.0 / n2)


def draw(n1, n2, family, P=None, seed=20261018):
    """-> A1, A2, d (float64 arrays of multiples of 1/8)."""
    fam = {"benign": 0, "separated": 1}[family]
    P = P if P is not None else (P_BENIGN if fam == 0 else P_SEPARATED)
    rng = np.random.default_rng([seed, n1, n2, fam])
    A1 = rng.integers(1, 64, P) / 8.0
    A2 = rng.integers(1, 64, P) / 8.0
    if fam == 0:
        nh = _harmonic(n1, n2)
        # t = d / se, se = sqrt(A1^2 / n1 + A2^2 / n2), grows as sqrt(n) at a given shift: past 50 v 50 the largest shift is
        # 50 se (it shrinks as n^-1/2), or nearly half the columns of 2100 v 2100 would underflow (p < 1e-290, where only the
        # absolute term decides)
        se = np.sqrt(A1 * A1 / n1 + A2 * A2 / n2)
        hi = np.minimum(160.0, 50.0 * se) if nh > 25.0 else np.full(P, 160.0)
        d = np.exp(rng.uniform(math.log(0.1), np.log(np.maximum(hi, 0.125))))
        if nh > 25.0:
            # a larger share of very deep columns (1e-290 < p < 1e-100 is the narrow band 21 < t < 37 there): one in seven aims at it
            aim = np.arange(P) % 7 == 3
            d[aim] = (np.exp(rng.uniform(math.log(22.0), math.log(35.0), P)) * se)[aim]
        d = np.minimum(d, 60.0 * np.minimum(A1 * math.sqrt((n1 - n1 % 2) / n1), A2 * math.sqrt((n2 - n2 % 2) / n2)))
        d = np.maximum(np.floor(d * 8.0), 1.0) / 8.0
        d[::7] = 0.0
    else:
        lo = 70.0 * np.maximum(A1, A2)
        d = np.ceil(np.exp(rng.uniform(np.log(lo), math.log(1000.0))) * 8.0) / 8.0
        d = np.minimum(d, 1000.0)
        # the edge columns, at the end
        k = P - N_EDGE
        A1[k:k + 3] = 0.0; A2[k:k + 3] = 0.0                # both sets constant: NaN
        d[k + 2] = 0.0                                      # ... and equal
        A1[k + 3:k + 6] = 0.0                               # set 0 constant: nu = n2 - 1
        A2[k + 6:] = 0.0                                    # set 1 constant: nu = n1 - 1
        d[k + 5] = 0.125; d[k + 7] = 0.125                  # (a small t on that nu)
    return A1, A2, d


def column_values(n1, n2, A1, A2, d):
    """-> M[P, n1 + n2] (float64; every entry exact in float32)."""
    P = len(d)
    M = np.empty((P, n1 + n2), np.float64)
    for lo, n, A, h in ((0, n1, A1, 0.5 * d), (n1, n2, A2, -0.5 * d)):
        sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        if n % 2:
            sign[-1] = 0.0
        M[:, lo:lo + n] = A[:, None] * sign[None, :] + h[:, None]
    assert np.array_equal(M.astype(np.float32).astype(np.float64), M)
    return M


def positions_packed(P, first=1):
    return np.arange(P, dtype=np.int64) + first


def positions_spread(P, windows, first=1, window_bp=WINDOW):
    """The columns dealt round robin to the given windows of `window_bp` positions (window w starts at first + w * window_bp),
    packed from the start of each."""
    windows = np.asarray(windows, np.int64)
    k = np.arange(P, dtype=np.int64)
    return first + windows[k % len(windows)] * window_bp + k // len(windows)


def columns_to_runlists(M, positions=None, dtype=np.float32):
    """M[P, N]: track i has the 1-bp run [pos[p], pos[p] + 1) of value M[p, i] -- from arrays (no Python loop over runs)."""
    M = np.asarray(M, np.float64)
    P, N = M.shape
    pos = positions_packed(P) if positions is None else np.asarray(positions, np.int64)
    order = np.argsort(pos, kind="stable")
    pos, M = pos[order], M[order]
    assert P == 0 or (np.diff(pos) > 0).all()
    seg_off = np.arange(N + 1, dtype=np.int64) * P
    start = np.tile(pos.astype(np.int32), N)
    return RunLists(1, N, seg_off, start, start + 1, np.ascontiguousarray(M.T).reshape(-1).astype(dtype))


def bound(t, nu, p_ref):
    """What tests/test_tdist_fast.py::test_fast_tail_against_mpmath allows the device's form compiled for the host: 1e-12 + 1e-15 nu
    relative (a * log(x) with a = nu / 2: x is itself rounded), and below t = 3 (nu <= 2000), where the fraction is taken in y and
    the result is 1 - r, the front factor's a * 1e-16 as an absolute error."""
    t, nu, p_ref = (np.asarray(x, np.float64) for x in (t, nu, p_ref))
    wide = np.where((t < 3.0) & (nu <= 2000.0), 3e-16 * (nu / 2 + 8.0), 0.0)
    return (1e-12 + 1e-15 * nu) * p_ref + 1e-300 + wide


def p_reference(t, nu):
    """2 Q(t; nu) = I_x(nu / 2, 1 / 2), x = nu / (nu + t^2), of the f64 pair (t, nu) as it stands, in 40 digits; NaN where
    either is NaN."""
    import mpmath as mp
    out = np.full(len(t), np.nan)
    with mp.workdps(40):
        half = mp.mpf("0.5")
        for k, (a, b) in enumerate(zip(t, nu)):
            if math.isnan(a) or math.isnan(b):
                continue
            if a == 0.0:
                out[k] = 1.0
                continue
            T, NU = mp.mpf(float(a)), mp.mpf(float(b))
            out[k] = float(mp.betainc(NU / 2, half, 0, NU / (NU + T * T), regularized=True))
    return out


class Columns:
    """One set of columns and its reference: t, nu (the oracle's, f64), p_ref (mpmath on those), nan (where the reference
    answers NaN: var1 + var2 == 0 or nu NaN)."""

    def __init__(self, oracle, n1, n2, family, P=None):
        self.n1, self.n2, self.family = n1, n2, family
        self.A1, self.A2, self.d = draw(n1, n2, family, P)
        self.M = column_values(n1, n2, self.A1, self.A2, self.d)
        P = len(self.d)
        ones = np.ones(n1 + n2, np.uint8)
        tn = np.array([oracle.ttest_stat(n1, n2, self.M[p], ones) for p in range(P)], np.float64).reshape(P, 2)
        self.t, self.nu = tn[:, 0].copy(), tn[:, 1].copy()
        constant = (self.A1 * (n1 > 1) == 0.0) & (self.A2 * (n2 > 1) == 0.0)      # var1 + var2 == 0 (setComparisons.c:98)
        self.t[constant] = np.nan
        self.nan = np.isnan(self.t) | np.isnan(self.nu)
        self.p_ref = p_reference(np.where(self.nan, np.nan, self.t), self.nu)
        self.bound = bound(self.t, self.nu, self.p_ref)

    def __len__(self):
        return len(self.d)

    def runlists(self, positions=None, dtype=np.float32):
        return columns_to_runlists(self.M, positions, dtype)

    def ratio(self, values):
        """|values - p_ref| / bound per column (NaN where the reference is NaN); the NaN positions must match."""
        values = np.asarray(values, np.float64)
        assert np.array_equal(np.isnan(values), self.nan), ("NaN positions", np.flatnonzero(np.isnan(values) != self.nan)[:8])
        with np.errstate(invalid="ignore"):
            return np.abs(values - self.p_ref) / self.bound

    def classes(self):
        """Masks of the regions of wt_tdist_2Q_fast (csrc/wt_core.h) a column's (t, nu) falls in."""
        a = self.nu / 2
        ok = ~self.nan
        with np.errstate(invalid="ignore"):
            t2 = self.t * self.t
            inv = 1.0 / (self.nu + t2)
            x = self.nu * inv
            textbook = ~(x * (a + 0.5 + 2) < a + 1)
            seam = (t2 < 9.0) & (a <= 1000.0)
            nz = self.t > 0
            return {
                "a<16": ok & nz & (a < 16.0),
                "textbook": ok & nz & textbook,
                "seam-only": ok & nz & ~textbook & seam,
                "x-side": ok & nz & ~textbook & ~seam,
                "a>1000": ok & nz & (a > 1000.0),
                "deep": ok & (self.p_ref > 0) & (self.p_ref < 1e-100),
                "t==0": ok & (self.t == 0),
            }


CLASS_NAMES = ["a<16", "textbook", "seam-only", "x-side", "a>1000", "deep", "t==0"]

_cache = {}


def columns(oracle, n1, n2, family, P=None):
    """Computed once per session and shared; callers leave it unchanged."""
    key = (n1, n2, family, P)
    if key not in _cache:
        _cache[key] = Columns(oracle, n1, n2, family, P)
    return _cache[key]
