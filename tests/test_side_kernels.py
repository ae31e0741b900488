"""The stand-alone passes around the reducers -- csrc/wt_moments.hip, csrc/wt_compress.hip, csrc/wt_map.hip and
wt_auc_kernel / wt_pearson_kernel of csrc/wt_moments.hip -- at every seam of their launch geometry, against references that
are exact (tests/exact.py) or pinned on the compiled reference (oracle.compress, oracle.map_values).

These are plain .hip translation units the CPU emulator never compiles: a GPU test is their only guard, and the older ones run
at sizes where most of the machinery idles (a few 4096-run tiles for the map scan whose carry starts after 64; five leaders
for the compression's 131 072-run blocks; one benign list for the moments).  Every size below is derived from a constant of
the code, cited where it is used: if the constant changes, the list is visibly stale.

CPU tests (unmarked) check the references themselves; `-m gpu` drives the product through its Python mirrors."""
import ctypes as C

import numpy as np
import pytest

import exact
from exact import rel_err, same_bits

gpu = pytest.mark.gpu

# The issue's conditioning classes (mean, dev) for T = S L (v - mean)^2; the last one lies BEYOND the reference: the f64
# run-by-run update has lost its digits there, the kernel's pivots are claimed not to (wt_moments.hip header).
CLASSES = {"1": (1.0, 1.0), "1e3": (1e3, 1.0), "1e5": (1e5, 1.0), "small": (1e-6, 1e-7), "1e8": (1e8, 1.0)}
N_COND = 3_000_000
REL = 1e-9              # the project's bound for fused integrators -- here relative to |exact|, not to max(1, ...)
BEYOND = 1e-6           # BASELINE.json: float statistics, relative


def _need_long_double():
    if not exact.long_double_ok():
        pytest.skip("np.longdouble is a plain double here: no reference better than f64 above %d runs" % exact.FRACTION_MAX)


# =====================================================================================================================
# 0. the references (CPU)
# =====================================================================================================================
@pytest.mark.parametrize("ratio", [1.0, 1e3, 1e5, 1e6, 1e8, 1e9, "small"])
def test_long_double_against_fraction(ratio):
    """The corrected two-pass long-double sums against exact rational arithmetic on 2e4 runs of every conditioning class
    (and the two of the issue's table beyond them): at most 4 ulp of f64 in sum, span and T."""
    _need_long_double()
    mean, dev = (1e-6, 1e-7) if ratio == "small" else (ratio, 1.0)
    s, f, v = exact.conditioned(11, 20_000, mean, dev)
    v[::97] = np.nan
    fr = exact.moments_exact(s, f, v, "fraction")
    ld = exact.moments_exact(s, f, v, "longdouble")
    for name, a, b in zip(("sum", "span", "T"), ld, fr):
        assert abs(a - b) <= 4 * np.spacing(abs(b)), (ratio, name, a, b)
    assert same_bits(ld[3], fr[3]) and same_bits(ld[4], fr[4])


def test_pearson_long_double_against_fraction():
    _need_long_double()
    rng = np.random.default_rng(5)
    s, f, _ = exact.conditioned(12, 20_000, 0, 1)
    vals = np.stack([1e3 + rng.standard_normal(20_000), -40 + 3 * rng.standard_normal(20_000)], axis=1)
    ip = (rng.random((20_000, 2)) < 0.9).astype(np.uint8)
    mf, rf = exact.pearson_exact(s, f, vals, ip, [0.5, -2.0], "fraction")
    ml, rl = exact.pearson_exact(s, f, vals, ip, [0.5, -2.0], "longdouble")
    for a, b in zip(ml, mf):
        assert abs(a - b) <= 4 * np.spacing(abs(b)), (ml, mf)
    assert abs(rl - rf) <= 4 * np.spacing(abs(rf))


@pytest.mark.parametrize("ratio", [1.0, 1e3])
def test_sequential_against_exact(ratio):
    """Where the reference's own f64 update is still good (mean/dev <= 1e3) it agrees with exact to 1e-11: the two kinds of
    reference do not contradict each other where both apply."""
    from test_integrator_moments import _sequential
    s, f, v = exact.conditioned(13, 20_000, ratio, 1.0)
    T, total, count, mn, mx = _sequential(s, f, v)
    e = exact.moments_exact(s, f, v, "fraction")
    assert rel_err(T, e[2]) <= 1e-11 and rel_err(total, e[0]) <= 1e-11, (T, total, e)
    assert count == e[1] and same_bits(mn, e[3]) and same_bits(mx, e[4])


def test_compiled_sequential_is_the_python_one():
    """tests/seq_moments.c restates _sequential operation for operation: the same bits, NaN runs, signed zeros and a
    badly conditioned list included (the bounds of the GPU tests are multiples of ITS error)."""
    from test_integrator_moments import _sequential
    for seed, (mean, dev) in enumerate([(1.0, 1.0), (1e6, 1.0), (1e-6, 1e-7), (0.0, 1.0)]):
        s, f, v = exact.conditioned(20 + seed, 5000, mean, dev)
        v[::13] = np.nan
        v[5], v[6] = 0.0, -0.0
        want, got = _sequential(s, f, v), exact.seq_moments(s, f, v)
        assert all(same_bits(a, float(b)) for a, b in zip(got, want)), (seed, got, want)
    got = exact.seq_moments(s[:3], f[:3], np.full(3, np.nan))
    assert got[:3] == (0.0, 0.0, 0.0) and np.isnan(got[3]) and np.isnan(got[4])


def test_first_occurrence_rule_of_the_exact_reference():
    """min / max of moments_exact keep the FIRST run that reaches the extreme, like the reference's strict < / >."""
    from test_integrator_moments import _sequential
    s, f = np.arange(1, 9, dtype=np.int32), np.arange(2, 10, dtype=np.int32)
    for v in ([1, 0.0, 2, -0.0, 3, np.nan, 0.0, 1], [1, -0.0, 2, 0.0, 3, np.nan, 0.0, 1], [-1, np.nan, -0.0, 0.0, -2, -2, -0.0, -1],
              [np.nan, -1, 0.0, -0.0, -2, -2, -0.0, -1]):
        v = np.array(v, np.float64)
        _, _, _, mn, mx = _sequential(s, f, v)
        e = exact.moments_exact(s, f, v)
        assert same_bits(e[3], mn) and same_bits(e[4], mx), (v, e, mn, mx)


def test_exact_by_construction_sums_in_any_order():
    """The generator's promise: f64 sums of L * v in three different orders are the integer sum, bit for bit."""
    rng = np.random.default_rng(3)
    for n, signed in ((1, False), (1000, True), (2_000_000, True), (2_000_001, False)):
        s, f, v, eighths = exact.exact_by_construction(rng, n, signed=signed, nan_prob=0.05)
        ok = ~np.isnan(v)
        p = ((f.astype(np.int64) - s).astype(np.float64) * v)[ok]
        forward = float(np.cumsum(p)[-1])                   # strictly sequential
        backward = float(np.cumsum(p[::-1])[-1])
        pairwise = float(p[rng.permutation(len(p))].sum())  # NumPy's pairwise blocks over a shuffle
        want = eighths / 8.0
        assert float(eighths) == eighths and want * 8 == eighths
        assert forward == want and backward == want and pairwise == want, (n, forward, backward, pairwise, want)
        assert np.all(np.diff(s) > 0) and np.all(f[:-1] <= s[1:]) and np.all(f > s)


def _seq_err(s, f, v):
    """(error in T, error in sum) of the f64 run-by-run update against exact, and the exact moments"""
    e = exact.moments_exact(s, f, v)
    T, total = exact.seq_moments(s, f, v)[:2]
    return rel_err(T, e[2]), rel_err(total, e[0]), e


def test_sequential_update_has_lost_its_digits_at_1e8():
    """The class `1e8` of test_gpu_moments_conditioning documents itself: on that very list (the compiled run-by-run update
    over all 3e6 runs, no prefix) the reference's arithmetic is off by more than the 1e-6 the device is held to, while at
    mean/dev = 1e3 it is still far inside."""
    _need_long_double()
    eT, es, _ = _seq_err(*exact.conditioned(108, N_COND, *CLASSES["1e8"]))
    print("sequential f64 update, 3e6 runs, mean/dev 1e8: relative error in T %.3g, in sum %.3g" % (eT, es))
    assert eT > BEYOND, eT
    eT3, _, _ = _seq_err(*exact.conditioned(103, N_COND, *CLASSES["1e3"]))
    assert eT3 < 1e-9, eT3


# ---- the special values of the map operators: the expectation itself is pinned on the compiled operator iterators ----
MAP_TABLE_OPS = [("scale", -2.5), ("scale", 0.0), ("offset", 3.25), ("ln", 0.0), ("log", 2.0), ("log", 10.0), ("exp", 0.0),
                 ("expb", 2.0), ("expb", 10.0), ("pow", 2.0), ("pow", 3.0), ("pow", -1.0), ("pow", -2.0), ("pow", 0.5),
                 ("pow", -0.5), ("pow", 0.0), ("abs", 0.0), ("gt", 12.5), ("gte", 12.5), ("lt", 12.5), ("lte", 12.5)]
TRANSCENDENTAL = ("ln", "log", "exp", "expb", "pow")


def _map_table(dt):
    """+-0, the comparisons' threshold and its two neighbours, the smallest and largest denormal, FLT_MAX (and DBL_MAX),
    +-inf, NaN, negative bases, arguments on which exp overflows.  (No argument whose RESULT would be a denormal of a
    transcendental: 1e-12 relative is not a statement about one ulp of 4.9e-324.)"""
    fi, f32 = np.finfo(dt), np.finfo(np.float32)
    thr = dt(12.5)
    vals = [0.0, -0.0, fi.smallest_subnormal, -fi.smallest_subnormal, np.nextafter(fi.tiny, dt(0)), fi.tiny, f32.max, -f32.max,
            fi.max, -fi.max, np.inf, -np.inf, np.nan, thr, np.nextafter(thr, dt(np.inf)), np.nextafter(thr, dt(-np.inf)),
            1.0, -1.0, 0.5, -0.5, 2.0, -2.0, 3.0, -3.0, 1.5, -1.5, 4.0, 0.25, 88.0, 89.0, 308.0, 309.0, 700.0, 709.5, 710.0, 1e3,
            -700.0, -800.0, -1e3, 1e-30, 1e30]
    return np.array(vals, dt)


@pytest.mark.parametrize("op,param", MAP_TABLE_OPS)
def test_map_special_values_oracle_vs_compiled_reference(oracle, op, param):
    """oracle.map_values on the table of special values == the compiled reference's operator iterator over a track that
    holds them: values bit for bit (NaN for NaN), the same runs dropped."""
    if not oracle.have_ref():
        pytest.skip("compiled reference not available")
    for dt in (np.float32, np.float64):
        v = _map_table(dt).astype(np.float64)
        s = np.arange(1, 2 * len(v), 2, dtype=np.int32)
        d = dict(n_chrom=1, n_tracks=1, seg_off=np.array([0, len(v)], np.int64), start=s, finish=s + 1, value=v,
                 defaults=np.zeros(1))
        out, keep = oracle.map_values(op, param, v)
        k = keep != 0
        rc, rs, rf, rv, rd = oracle.ref_map(d, 0, op, param)
        assert np.array_equal(rs, s[k]) and np.array_equal(rf, s[k] + 1), (op, param, dt)
        assert _bits_equal(rv, out[k]), (op, param, dt, rv, out[k])


def _bits_equal(a, b):
    """element for element the same doubles: -0.0 is not 0.0; NaN equals NaN whatever its sign"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    m = ~np.isnan(a)
    return bool(np.array_equal(a[m].view(np.int64), b[m].view(np.int64)))


# =====================================================================================================================
# GPU plumbing
# =====================================================================================================================
@pytest.fixture(scope="module")
def engine():
    import torch
    assert torch.cuda.is_available()
    from wiggletools_amd import engine as E
    return E


def _runs(engine, s, f, v, off=0, tail=None, cro=None):
    """DeviceRuns over the three arrays, as views that begin `off` elements into their allocations (off = 1: start / finish
    are no longer 8-aligned and value no longer 16-aligned -> wt_moments_kernel's scalar loads) and are followed by the
    `tail` triple, which no kernel may read.  What lies before and after the view is poison."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    ts, tf, tv = tail if tail is not None else (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    n = len(s)

    def up(a, t, dtype, poison):
        h = np.concatenate([np.full(off, poison, dtype), np.asarray(a, dtype), np.asarray(t, dtype), np.full(1, poison, dtype)])
        d = torch.from_numpy(h).to(dev)
        assert d.data_ptr() % 16 == 0
        return d[off:off + n + len(t)]
    cro = np.array([0, n], np.int64) if cro is None else np.asarray(cro, np.int64)
    r = engine.DeviceRuns(up(s, ts, np.int32, -(2 ** 30)), up(f, tf, np.int32, 2 ** 30), up(v, tv, np.float64, 1e300),
                          torch.from_numpy(cro).to(dev))
    r.n = n
    return r


def _sixteenths(s, f, v):
    """(sum, span) of a list whose values are multiples of 1/16, by integer arithmetic"""
    ok = ~np.isnan(v)
    q = np.rint(v[ok] * 16).astype(np.int64)
    assert np.array_equal(q / 16.0, v[ok])
    L = (f.astype(np.int64) - s)[ok]
    return int((L * q).sum()) / 16.0, float(L.sum())


# =====================================================================================================================
# 1. wt_moments.hip through wtamd_runs_moments
# =====================================================================================================================
# wt_moments.hip: WM_BLOCK 256 lanes, two runs per lane and load, blocks = ceil(n / 2048) (2 * WM_BLOCK * 4) capped at
# WM_MAX_BLOCKS 2048; wt_moments_final_kernel: 256 lanes, per = ceil(blocks / 256) partials each.
WM_BLOCK, WM_RUNS_PER_BLOCK, WM_MAX_BLOCKS = 256, 2048, 2048
MOMENT_SIZES = ([0, 1, 2, 3, WM_BLOCK - 1, WM_BLOCK, WM_BLOCK + 1, 2 * WM_BLOCK - 1, 2 * WM_BLOCK, 2 * WM_BLOCK + 1,
                 WM_RUNS_PER_BLOCK - 1, WM_RUNS_PER_BLOCK, WM_RUNS_PER_BLOCK + 1]
                + [WM_RUNS_PER_BLOCK * k + d for k in (255, 256, 257) for d in (-1, 1)]      # final kernel: per 1 -> 2 at 257 blocks
                + [2 * WM_RUNS_PER_BLOCK * WM_MAX_BLOCKS + 3])         # the cap holds, every lane strides, the tail is scalar


def _check_exact_list(engine, s, f, v, off, what, tail=None):
    """sum, span, min, max bit for bit; T to 1e-9 of |exact|; the same six doubles twice"""
    r = _runs(engine, s, f, v, off, tail)
    m = r.moments()
    want_sum, want_span = _sixteenths(s, f, v)
    e = exact.moments_exact(s, f, v)
    assert want_sum == e[0] and want_span == e[1]           # (two exact references agree)
    assert same_bits(m[0], want_sum) or (m[0] == 0 and want_sum == 0), (what, "sum", m[0], want_sum)
    assert m[1] == want_span, (what, "span", m[1], want_span)
    assert same_bits(m[3], e[3]) and same_bits(m[4], e[4]), (what, "min/max", m[3], m[4], e[3], e[4])
    assert rel_err(m[2], e[2]) <= REL, (what, "T", m[2], e[2])
    assert m[5] == 0.0 and r.moments().tobytes() == m.tobytes(), what
    return m


@gpu
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", MOMENT_SIZES)
def test_gpu_moments_sizes(engine, n, off):
    """Exact-by-construction lists (NaN runs sprinkled in) at every seam of the launch, wide loads (off 0; odd n: the last
    run goes to the scalar tail) and scalar loads (off 1)."""
    if n > exact.FRACTION_MAX:
        _need_long_double()
    s, f, v, _ = exact.exact_by_construction(np.random.default_rng(n), n, signed=True, nan_prob=0.03)
    _check_exact_list(engine, s, f, v, off, "n=%d off=%d" % (n, off))


# (name, n, i, j): where the two zeros sit.  Wide path, `blocks` blocks of 256 lanes: pair q = (2q, 2q + 1) goes to lane
# q mod lanes in stride q div lanes, lanes = 256 * blocks.
_FINAL_N = WM_RUNS_PER_BLOCK * 600          # 600 blocks: the final kernel's lanes take 3 partials each
TIE_PLACES = [
    ("same pair", 4096, 10, 11),
    ("same lane, two strides", 4096, 10, 10 + 2 * 512),                 # n 4096: 2 blocks, 512 lanes, 4 strides
    ("two lanes of a wavefront", 4096, 6, 80),
    ("two wavefronts of a block", 4096, 6, 200),
    ("two blocks", 4096, 6, 600),
    ("two partials of one final-kernel lane", _FINAL_N, 10, 2 * WM_BLOCK + 10),           # blocks 0 and 1
    ("two lanes of the final kernel", _FINAL_N, 10, 2 * (WM_BLOCK * 10 + 5)),             # blocks 0 and 10
    ("two wavefronts of the final kernel", _FINAL_N, 10, 2 * (WM_BLOCK * 300 + 5)),       # blocks 0 and 300
    ("wide element and scalar tail, one lane", 4097, 0, 4096),
    ("wide element and scalar tail, two lanes", 4097, 10, 4096),
]


@gpu
@pytest.mark.parametrize("place", TIE_PLACES, ids=[p[0].replace(" ", "_").replace(",", "") for p in TIE_PLACES])
def test_gpu_moments_first_occurrence_ties(engine, place):
    """All values >= 0 (<= 0 for max) with one +0.0 and one -0.0: the sign of min / max is that of the EARLIER run, in both
    orders, on the wide and on the scalar path.  Then a non-zero extreme that occurs twice, with a NaN between the two."""
    name, n, i, j = place
    if n > exact.FRACTION_MAX:
        _need_long_double()
    rng = np.random.default_rng(n + i)
    s, f, base, _ = exact.exact_by_construction(rng, n, levels=100)
    base = base + 0.125                                     # everything > 0
    for kind, sign in (("min", 1.0), ("max", -1.0)):
        for first, second in ((0.0, -0.0), (-0.0, 0.0)):
            for off in (0, 1):
                v = sign * base
                v[i], v[j] = first, second
                m = _check_exact_list(engine, s, f, v, off, (name, kind, first, off))
                got = m[3] if kind == "min" else m[4]
                assert got == 0 and np.signbit(got) == np.signbit(first), (name, kind, first, second, off, got)
        v = sign * base
        v[i] = v[j] = sign * 0.0625
        if j - i > 1:
            v[(i + j) // 2] = np.nan
        m = _check_exact_list(engine, s, f, v, 0, (name, kind, "twice"))
        assert (m[3] if kind == "min" else m[4]) == sign * 0.0625


@gpu
@pytest.mark.parametrize("lead", ["first", "256", "300", "all"])
def test_gpu_moments_pivot_behind_nan_runs(engine, lead):
    """The launch's pivot K is the first value among the list's first 256 runs, 0 when they are all NaN; an all-NaN list has
    no moments at all, and wtamd_moments_finish makes of it what the reference's closing arithmetic makes of a source without
    a run (T / (0 - 1) = -0.0 and so on)."""
    from test_integrator_moments import _closing
    n = 10_001                                              # 5 blocks, odd
    for off in (0, 1):
        s, f, v, _ = exact.exact_by_construction(np.random.default_rng(7), n, signed=True, nan_prob=0.02)
        k = {"first": 1, "256": WM_BLOCK, "300": 300, "all": n}[lead]
        v[:k] = np.nan
        m = _check_exact_list(engine, s, f, v, off, (lead, off))
        if lead != "all":
            continue
        assert m[0] == 0 and m[1] == 0 and m[2] == 0 and np.isnan(m[3]) and np.isnan(m[4]), m
        r = _runs(engine, s, f, v, off)
        got = {"var": r.var(), "stddev": r.stddev(), "cv": r.cv(), "max": r.max(), "min": r.min(), "span": r.span()}
        for kind in ("var", "stddev", "cv"):
            assert same_bits(got[kind], _closing(0.0, 0.0, 0, kind)), (kind, got[kind])
        assert same_bits(got["var"], -0.0) and np.isnan(got["cv"]) and np.isnan(got["max"]) and np.isnan(got["min"])
        assert got["span"] == 0.0


def _held_to_the_sequential_update(m, s, f, v, what):
    """The issue's rule: the device's relative error in T and in sum against exact is at most max(4 x the error of the f64
    run-by-run update on the same list, 1e-9) -- 4: a different but equally valid rounding order."""
    eT, es, e = _seq_err(s, f, v)
    dT, ds = rel_err(m[2], e[2]), rel_err(m[0], e[0])
    print("moments %s: T exact %.17g device error %.3g (sequential %.3g); sum device error %.3g (sequential %.3g)"
          % (what, e[2], dT, eT, ds, es))
    assert m[1] == e[1] and same_bits(m[3], e[3]) and same_bits(m[4], e[4]), (what, m, e)
    return dT, ds, eT, es


@gpu
def test_gpu_moments_pivot_is_an_outlier(engine):
    """The first run -- the launch's pivot -- is a 1-bp outlier 10^6 deviations away from everything else."""
    s, f, v = exact.conditioned(31, 10_001, 100.0, 1.0)
    s[0] = f[0] - 1
    v[0] = 100.0 + 1e6
    for off in (0, 1):
        m = _runs(engine, s, f, v, off).moments()
        dT, ds, eT, es = _held_to_the_sequential_update(m, s, f, v, "outlier pivot, off %d" % off)
        assert dT <= max(4 * eT, REL) and ds <= max(4 * es, REL)
    # and the T of everything BUT the outlier is not lost in it: the same list with the outlier's run NaN'd out, K unchanged in
    # spirit (the next run becomes the pivot), must still satisfy the rule
    v[0] = np.nan
    m = _runs(engine, s, f, v, 0).moments()
    dT, ds, eT, es = _held_to_the_sequential_update(m, s, f, v, "outlier removed")
    assert dT <= max(4 * eT, REL) and ds <= max(4 * es, REL)


@gpu
@pytest.mark.parametrize("cls", list(CLASSES))
def test_gpu_moments_conditioning(engine, cls):
    """3e6 runs of length 1 .. 49, values mean + dev * N(0, 1).  Held to max(4 x the error of the f64 run-by-run update,
    1e-9) RELATIVE TO |exact| (class `small`, T ~ 1e-6: an absolute tolerance would pass anything).  The run-by-run update
    is the compiled restatement (tests/seq_moments.c) over the whole list, not a prefix.  Class `1e8` lies beyond the
    reference (test_sequential_update_has_lost_its_digits_at_1e8): there the device is held to 1e-6 of exact -- the claim of
    wt_moments.hip's header about its two pivots.
    Measured on an MI355X, relative error against exact of the device / of the run-by-run f64 update:
        class 1      T 2.0e-16 / 3.6e-14    sum 2.0e-16 / 6.4e-14
        class 1e3    T 0       / 6.0e-14    sum 0       / 4.7e-14
        class 1e5    T 0       / 8.1e-10    sum 0       / 1.8e-14
        class small  T 0       / 9.3e-15    sum 0       / 5.4e-14
        class 1e8    T 0       / 1.5e-3     sum 0       / 1.4e-14
    (0: the device's double is the one nearest the exact value.)"""
    _need_long_double()
    mean, dev = CLASSES[cls]
    seed = {"1": 101, "1e3": 103, "1e5": 105, "small": 107, "1e8": 108}[cls]
    s, f, v = exact.conditioned(seed, N_COND, mean, dev)
    m = _runs(engine, s, f, v).moments()
    dT, ds, eT, es = _held_to_the_sequential_update(m, s, f, v, "class %s" % cls)
    if cls == "1e8":
        assert eT > BEYOND, eT
        assert dT <= BEYOND and ds <= BEYOND, (dT, ds)
    else:
        assert dT <= max(4 * eT, REL) and ds <= max(4 * es, REL), (dT, eT, ds, es)


@gpu
@pytest.mark.parametrize("n", [1000, 1001, 4097])
def test_gpu_moments_n_smaller_than_the_arrays(engine, n):
    """moments(n=...) over arrays that go on: NaN, huge values and zero lengths past n are not read into the result."""
    s, f, v, _ = exact.exact_by_construction(np.random.default_rng(n), n, signed=True, nan_prob=0.03)
    ts = np.full(3000, s[-1] + 100, np.int32)
    tf = ts.copy()                                          # zero lengths ...
    tf[1::3] += 1000
    tv = np.tile([np.nan, 1e300, -1e300], 1000)
    for off in (0, 1):
        r = _runs(engine, s, f, v, off, tail=(ts, tf, tv))
        assert r.start.numel() == n + 3000
        m = r.moments(n=n)
        want_sum, want_span = _sixteenths(s, f, v)
        e = exact.moments_exact(s, f, v)
        assert same_bits(m[0], want_sum) and m[1] == want_span and same_bits(m[3], e[3]) and same_bits(m[4], e[4]), (n, off, m, e)
        assert rel_err(m[2], e[2]) <= REL


# =====================================================================================================================
# 2. wt_compress.hip through DeviceRuns.compress()
# =====================================================================================================================
# wt_compress.hip: bit r of word r / 64; WC_BLOCK 256 runs per classify / resolve block; WC_WORDS_PER_BLOCK 2048 words =
# 131 072 runs per wc_count / wc_emit block.
WC_WORD, WC_BLOCK, WC_SEAM = 64, 256, 2048 * 64
WC_MAX_CHAIN = 4096     # one lane of wc_resolve walks an uncertain chain serially: no test builds a longer one


def _sure_leaders(c, s, f, v):
    """wc_classify's SURE LEADER restated: other chromosome, not contiguous, NaN-ness differs, |dv| >= 2.000001e-6"""
    with np.errstate(invalid="ignore"):
        d = np.abs(v[1:] - v[:-1])
    nn = np.isnan(v)
    sure = (c[1:] != c[:-1]) | (s[1:] != f[:-1]) | (nn[1:] != nn[:-1]) | (~nn[1:] & ~nn[:-1] & (d >= 2.000001e-6))
    return np.concatenate([[True], sure])


def _drift_list(seed, n, chains=(), const=()):
    """The drift recipe of test_gpu_run_compression_matches_reference_rule at any size: consecutive differences of 0,
    +-4e-7, 7e-7, 9e-7, -6e-7 around a base that jumps every ~50 runs, exact repeats, NaN runs and gaps.
    chains: (P, back) -- a sure leader at P - back followed by contiguous steps of +4e-7 up to P + 12: every third run of it
    is promoted, the first one at P - back + 3.  const: (lo, hi) -- a constant contiguous stretch."""
    rng = np.random.default_rng(seed)
    L = rng.integers(1, 6, n).astype(np.int64)
    gap = rng.random(n) < 0.02
    gap[::4000] = True                                      # a sure leader at least every WC_MAX_CHAIN runs
    nan = rng.random(n) < 0.03
    base = np.round(rng.random(n // 50 + 1) * 100)[np.arange(n) // 50]
    step = rng.choice([0.0, 0.0, 4e-7, -4e-7, 7e-7, 9e-7, -6e-7], n)
    for P, back in chains:
        a, b = P - back, P + 13
        gap[a] = True; gap[a + 1:b] = False; gap[b] = True
        nan[a:b] = False
        base[a:b] = 50.0
        step[a] = 0.0; step[a + 1:b] = 4e-7
    for lo, hi in const:
        gap[lo + 1:hi] = False
        nan[lo:hi] = False
        base[lo:hi] = 7.0
        step[lo:hi] = 0.0
    # (the walk restarts at every base jump, so that it stays a drift of a few 1e-6 and the rounding of base + walk small)
    walk = np.cumsum(step)
    walk -= walk[np.arange(n) // 50 * 50]
    for P, back in chains:
        walk[P - back:P + 13] = 4e-7 * np.arange(back + 13)
    for lo, hi in const:
        walk[lo:hi] = 0.0
    v = np.where(nan, np.nan, base + walk)
    start = 1 + np.cumsum(gap * 3 + np.concatenate([[0], L[:-1]]))
    return start.astype(np.int32), (start + L).astype(np.int32), v


def _compress_and_compare(oracle, engine, c, s, f, v, n_chrom, what):
    cro = np.zeros(n_chrom + 1, np.int64)
    np.cumsum(np.bincount(c, minlength=n_chrom), out=cro[1:])
    sure = np.flatnonzero(_sure_leaders(c, s, f, v))
    assert np.diff(np.concatenate([sure, [len(s)]])).max() <= WC_MAX_CHAIN, what
    ec, es, ef, ev = oracle.compress(c, s, f, v)
    out = _runs(engine, s, f, v, cro=cro).compress()
    gc, gs, gf, gv = out.to_host()
    assert out.n == len(es), (what, out.n, len(es))
    assert np.array_equal(gs, es) and np.array_equal(gf, ef) and np.array_equal(gc, ec), what
    assert _bits_equal(gv, ev), what
    ecro = np.zeros(n_chrom + 1, np.int64)
    np.cumsum(np.bincount(ec, minlength=n_chrom), out=ecro[1:])
    assert np.array_equal(out.chrom_run_off.cpu().numpy(), ecro), what
    return es, ecro


@gpu
def test_gpu_compress_block_seams_and_chromosome_boundaries(oracle, engine):
    """620 000 runs (five counting / emitting blocks) of the drift recipe with uncertain chains placed across a 64-run word
    seam, a 256-run classify-block seam and the 131 072-run seam -- a promotion landing on the first run after the seam and on
    the last run before it -- and chromosome boundaries on a word seam, on block seams, inside constant contiguous stretches,
    around an empty chromosome and at r == n."""
    n = 620_000
    word, blk = WC_WORD * 1001, WC_BLOCK * 301
    assert word % WC_BLOCK and blk % WC_SEAM and n > 4 * WC_SEAM
    chains = [(word, 3), (word + 2 * WC_WORD, 4), (blk, 3), (blk + 2 * WC_BLOCK, 4), (WC_SEAM, 3), (3 * WC_SEAM, 4), (4 * WC_SEAM, 3)]
    b_word, b_blk, b_seam, b_in = WC_WORD * 3001, WC_BLOCK * 1201, 2 * WC_SEAM, 400_010
    const = [(b_word - 20, b_word + 20), (b_seam - 20, b_seam + 20), (b_in - 20, b_in + 20)]
    s, f, v = _drift_list(42, n, chains, const)
    cro = np.array([0, b_word, b_seam, b_seam, b_blk, b_in, n, n])          # chromosome 2 and the last one are empty
    n_chrom = len(cro) - 1
    c = np.repeat(np.arange(n_chrom, dtype=np.int32), np.diff(cro))
    # the placed structures are what they are meant to be: contiguous, equal values across the constant boundaries; an
    # UNCERTAIN run (0 < |dv| < 2.000001e-6) promoted exactly at P / P - 1
    for b in (b_word, b_seam, b_in):
        assert s[b] == f[b - 1] and v[b] == v[b - 1] == 7.0
    es, ecro = _compress_and_compare(oracle, engine, c, s, f, v, n_chrom, "seams")
    lead = set(es.tolist())
    for P, back in chains:
        q = P - back + 3
        assert q in (P, P - 1) and s[q] == f[q - 1] and 0 < abs(v[q] - v[q - 1]) < 2.000001e-6
        assert int(s[q]) in lead and int(s[q - 1]) not in lead and int(s[q + 1]) not in lead, (P, back)
    for b in (b_word, b_seam, b_blk, b_in):
        assert int(s[b]) in lead, b                        # a chromosome start leads whatever the coordinates say
    assert ecro[2] == ecro[3] and ecro[-1] == ecro[-2] == len(es)


@gpu
@pytest.mark.parametrize("n", [1, WC_WORD - 1, WC_WORD, WC_WORD + 1, WC_SEAM - 1, WC_SEAM, WC_SEAM + 1])
def test_gpu_compress_sizes(oracle, engine, n):
    s, f, v = _drift_list(n, max(n, 100))
    s, f, v = s[:n], f[:n], v[:n]
    _compress_and_compare(oracle, engine, np.zeros(n, np.int32), s, f, v, 1, "n=%d" % n)
    if n > 1:       # ... and with the last run a chromosome of its own
        c = np.zeros(n, np.int32)
        c[-1] = 1
        _compress_and_compare(oracle, engine, c, s, f, v, 3, "n=%d, last run alone" % n)


@gpu
def test_gpu_compress_values_at_the_edges_of_the_rule(oracle, engine):
    """Short contiguous groups whose steps sit on the rule's edges -- |dv| of exactly 1e-6, 1e-6 +- 1 ulp, 2.000001e-6 +- 1
    ulp (the classifier's own threshold, against the predecessor), magnitudes where one ulp exceeds 1e-6, +-0.0, +-inf
    (inf - inf is NaN: the `<` fails) -- separated by gaps.  Expectations: oracle.compress only."""
    up, dn = lambda x: np.nextafter(x, np.inf), lambda x: np.nextafter(x, -np.inf)
    edges = [0.0, 1e-6, up(1e-6), dn(1e-6), 2.000001e-6, up(2.000001e-6), dn(2.000001e-6), 5e-7, 9.99999e-7, 1.5e-6, 2e-6, 3e-6]
    edges = edges + [-e for e in edges[1:]]
    groups = []
    for L0 in (0.0, -0.0, 1.0, -3.5, 1e-6, 255.0, 1e10, 1e12, -1e10):      # (ulp(1e10) = 1.9e-6, ulp(1e12) = 1.2e-4)
        for a in edges:
            for b in edges:
                groups.append([L0, L0 + a, L0 + a + b, L0 + b])
        for a in (up(L0), dn(L0), up(up(L0)), dn(dn(L0))):
            groups.append([L0, a, L0, a, up(a)])
    inf = np.inf
    groups += [[0.0, -0.0, 0.0], [-0.0, 0.0, 1e-7, -0.0], [inf, inf], [inf, inf, inf, 1.0], [-inf, -inf], [inf, -inf, inf], [1.0, inf, inf, 1.0],
               [np.nan, inf, np.nan, np.nan, inf], [1e308, inf], [-1e308, -inf, -inf]]
    rng = np.random.default_rng(9)
    for _ in range(3000):                                   # random walks over the edge steps
        k = int(rng.integers(3, 12))
        groups.append((float(rng.choice([0.0, 1.0, 77.0, 1e10])) + np.cumsum(rng.choice(edges, k))).tolist())
    v = np.array([x for g in groups for x in g], np.float64)
    first = np.zeros(len(v), bool)
    first[np.cumsum([0] + [len(g) for g in groups[:-1]])] = True
    L = rng.integers(1, 4, len(v))
    s = 1 + np.cumsum(first * 2 + np.concatenate([[0], L[:-1]]))
    s, f = s.astype(np.int32), (s + L).astype(np.int32)
    assert len(v) > 2 * WC_BLOCK * 20
    es, _ = _compress_and_compare(oracle, engine, np.zeros(len(v), np.int32), s, f, v, 1, "edges")
    assert len(groups) < len(es) < len(v)                   # (some steps merged, some led)


@gpu
def test_gpu_compress_capacity(oracle, engine):
    """An `out` smaller than the merged count: WtamdError, and nothing is written beyond `capacity` (guard elements behind
    every output array); a capacity of exactly the merged count succeeds."""
    import torch
    from wiggletools_amd import _lib
    n = 2 * WC_SEAM + 1000
    s, f, v = _drift_list(77, n)
    c = np.zeros(n, np.int32)
    ec, es, ef, ev = oracle.compress(c, s, f, v)
    m = len(es)
    G = 4096
    assert m > 8 * G                                        # (a truncated output is cut well inside the list)
    src = _runs(engine, s, f, v)
    dev = src.start.device
    for cap in (m, m - 1, m // 2, 1):
        bs = torch.full((cap + G,), -7, dtype=torch.int32, device=dev)
        bf = torch.full((cap + G,), -7, dtype=torch.int32, device=dev)
        bv = torch.full((cap + G,), -7.0, dtype=torch.float64, device=dev)
        out = engine.DeviceRuns(bs[:cap], bf[:cap], bv[:cap], torch.zeros(2, dtype=torch.int64, device=dev))
        assert out.as_struct().capacity == cap
        if cap == m:
            src.compress(out=out)
            assert out.n == m
            gc, gs, gf, gv = out.to_host()
            assert np.array_equal(gs, es) and np.array_equal(gf, ef) and _bits_equal(gv, ev)
        else:
            with pytest.raises(_lib.WtamdError):
                src.compress(out=out)
        torch.cuda.synchronize()
        assert bool((bs[cap:] == -7).all()) and bool((bf[cap:] == -7).all()) and bool((bv[cap:] == -7.0).all()), cap


# =====================================================================================================================
# 3. wt_map.hip
# =====================================================================================================================
# wt_map.hip: WM_TILE = WM_BLOCK 256 * WM_ITEMS 16 = 4096 runs per block; wm_scan_blocks scans 64 tile counts per step and
# carries into the next: one carry step per 64 * 4096 = 262 144 runs; wm_seg_offsets: 256 segment boundaries per block.
WM_TILE, WM_CARRY, WM_SEG_BLOCK = 4096, 64 * 4096, 256
N_MAP = 2 * WM_CARRY + 19 * WM_TILE + 1234                  # 603 346 runs, 148 tiles: three carry steps, a partial last tile
DROPPING = [("ln", 0.0), ("log", 2.0), ("gt", 12.5), ("gte", 12.5), ("lt", 12.5), ("lte", 12.5)]
KEEP_PATTERNS = ["all", "none", "half", "last of every tile", "first of every tile"]


def _pools(op, dt):
    thr = dt(12.5)
    up, dn = np.nextafter(thr, dt(np.inf)), np.nextafter(thr, dt(-np.inf))
    if op in ("ln", "log"):
        return [0.5, 1.0, 2.75, 1000.0, 2.0 ** -15, 1e30], [0.0, -0.0, -1.5, -1000.0, -np.inf]
    if op == "gt":
        return [up, 13.0, 1e6, np.inf], [thr, dn, -5.0, np.nan, -np.inf]
    if op == "gte":
        return [thr, up, 40.0, np.inf], [dn, -5.0, np.nan, -np.inf]
    if op == "lt":
        return [dn, -5.0, 0.0, -np.inf], [thr, up, np.nan, 1e9, np.inf]
    return [thr, dn, 0.0, -np.inf], [up, 1e9, np.nan, np.inf]


def _map_segments(n):
    """Segment boundaries exactly on tile seams, one before and one after, at n, hundreds of empty segments in a row, on
    both sides of the carry seams -- and more than 256 of them, so that the second block of wm_seg_offsets runs."""
    pts = [0, 0, 0, 1, WM_TILE - 1, WM_TILE, WM_TILE + 1, 2 * WM_TILE] + [2 * WM_TILE] * 300
    pts += [5 * WM_TILE + 77, WM_CARRY - 1, WM_CARRY, WM_CARRY + 1, WM_CARRY + WM_TILE, 100 * WM_TILE, 100 * WM_TILE + 1,
            2 * WM_CARRY - 1, 2 * WM_CARRY, 2 * WM_CARRY + 1, (n // WM_TILE) * WM_TILE, n - 1, n, n, n, n]
    seg = np.array(sorted(pts), np.int64)
    assert len(seg) > WM_SEG_BLOCK + 1 and seg[-1] == n
    return seg


def _map_case(rng, n, pattern, op, dt):
    keep = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "half": rng.random(n) < 0.5,
            "last of every tile": np.arange(n) % WM_TILE == WM_TILE - 1, "first of every tile": np.arange(n) % WM_TILE == 0}[pattern]
    kp, dp = _pools(op, dt)
    v = np.where(keep, rng.choice(np.array(kp, dt), n), rng.choice(np.array(dp, dt), n)).astype(dt)
    return keep, v


def _check_map(oracle, engine, t, op, param, what):
    """kept coordinates and seg_off bit-equal to the NumPy selection by the oracle's keep flags; values: 1e-12 relative for the
    transcendental operators (the module's existing bound: device libm), bit-equal for the others"""
    got = engine.map_runlists(t, op, param)
    out, keep = oracle.map_values(op, param, t.value.astype(np.float64))
    k = keep != 0
    exp_seg = np.concatenate([[0], np.cumsum(k)])[t.seg_off]
    assert np.array_equal(got.seg_off, exp_seg), what
    assert np.array_equal(got.start, t.start[k]) and np.array_equal(got.finish, t.finish[k]), what
    a, b = got.value, out[k]
    if op in TRANSCENDENTAL:
        assert np.array_equal(np.isnan(a), np.isnan(b)), what
        fin = ~np.isnan(b) & np.isfinite(b)
        assert _bits_equal(a[~fin], b[~fin]), what
        assert np.all(np.abs(a[fin] - b[fin]) <= 1e-12 * np.abs(b[fin])), (what, np.max(np.abs(a[fin] - b[fin]) / np.abs(b[fin])))
    else:
        assert _bits_equal(a, b), (what, a[:8], b[:8])
    return got, k


@gpu
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("op,param", DROPPING)
def test_gpu_map_compaction_across_carry_steps(oracle, engine, op, param, dt):
    """The operators that drop runs over 603 346 runs -- more than two carry steps of wm_scan_blocks -- under five keep
    patterns, with segment boundaries on, before and after the tile and carry seams, at n, and 300 empty segments in a row."""
    from wiggletools_amd.runlists import RunLists
    rng = np.random.default_rng(17)
    n = N_MAP
    assert n >= 600_000 and n > 2 * WM_CARRY
    L = rng.integers(1, 4, n)
    s = (1 + np.cumsum(np.concatenate([[0], L[:-1]]))).astype(np.int32)
    f = (s + L).astype(np.int32)                            # (sorted, non-overlapping across the whole list)
    seg = _map_segments(n)
    for pattern in KEEP_PATTERNS:
        keep, v = _map_case(rng, n, pattern, op, dt)
        t = RunLists(1, len(seg) - 1, seg, s, f, v)
        assert t.value.dtype == dt
        got, k = _check_map(oracle, engine, t, op, param, (op, pattern))
        assert np.array_equal(k, keep), (op, pattern)       # (the pools do what they were chosen for)
        if pattern == "none":
            assert len(got.start) == 0 and not got.seg_off.any()
        if pattern == "all":
            assert np.array_equal(got.seg_off, seg)


@gpu
@pytest.mark.parametrize("op,param", MAP_TABLE_OPS)
def test_gpu_map_special_values(oracle, engine, op, param):
    """engine.map_runlists on the table of special values (f32 and f64 input) against oracle.map_values, which
    test_map_special_values_oracle_vs_compiled_reference pins on the compiled operator iterators."""
    from wiggletools_amd.runlists import RunLists
    for dt in (np.float32, np.float64):
        v = _map_table(dt)
        s = np.arange(1, 2 * len(v), 2, dtype=np.int32)
        t = RunLists(1, 2, [0, 7, len(v)], s, s + 1, v)
        assert t.value.dtype == dt
        _check_map(oracle, engine, t, op, param, (op, param, dt.__name__))


# ---- per-track chains inside the pipeline: wm_chain_kernel, wm_compact_flag_kernel, wm_seg_offsets_flag ----
BIG_CHAINS = {
    "ln": lambda n: [[("ln", 0)]] * n,
    "gt": lambda n: [[("gt", 12.5)]] * n,
    "abs-log2": lambda n: [[("abs", 0), ("log", 2.0)]] * n,
    "mixed": None,                                          # test_mapiter.CHAINS[5]
    "f32-exact": lambda n: [[("abs", 0), ("scale", -1.0)]] * n,           # stays on wm_chain_kernel<float, float>
}


def _big_tracks(n_chrom):
    """8 float32 tracks of >= 4e5 runs each, values k/8 in [-60, 60] with zeros (ln / log drop them, exp stays finite)"""
    from wiggletools_amd.runlists import synth
    clens = [1_900_000] if n_chrom == 1 else [900_000, 1_000, 1_000_000]
    t = synth(8, clens, mean_run=4, gap_prob=0.1, seed=31 + n_chrom, dtype=np.float32, value_levels=480)
    rng = np.random.default_rng(n_chrom)
    t.value[:] = (t.value * rng.choice([1.0, -1.0, 0.0], size=len(t.value), p=[0.6, 0.3, 0.1])).astype(np.float32)
    return t


def _blocks_np(L, wi, names):
    """test_bwreader._blocks without the per-run Python objects: (chrom index, start, finish, value) arrays"""
    chrom, s, f, v = C.c_char_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    idx = {n: k for k, n in enumerate(names)}
    cc, ss, ff, vv = [np.zeros(0, np.int32)], [np.zeros(0, np.int32)], [np.zeros(0, np.int32)], [np.zeros(0)]
    while True:
        n = L.wtamd_iterator_next_block(wi, C.byref(chrom), C.byref(s), C.byref(f), C.byref(v))
        assert n >= 0
        if n == 0:
            return np.concatenate(cc), np.concatenate(ss), np.concatenate(ff), np.concatenate(vv)
        cc.append(np.full(n, idx[chrom.value.decode()], np.int32))
        ss.append(np.ctypeslib.as_array(C.cast(s, C.POINTER(C.c_int32)), shape=(n,)).copy())
        ff.append(np.ctypeslib.as_array(C.cast(f, C.POINTER(C.c_int32)), shape=(n,)).copy())
        vv.append(np.ctypeslib.as_array(C.cast(v, C.POINTER(C.c_double)), shape=(n,)).copy())


def _pipe_stats(L, wi):
    from wiggletools_amd.pipe import PipeStats
    st = PipeStats()
    L.wtamd_iterator_pipe_stats.restype = C.c_int
    L.wtamd_iterator_pipe_stats.argtypes = [C.c_void_p, C.POINTER(PipeStats)]
    assert L.wtamd_iterator_pipe_stats(wi, C.byref(st)) == 0
    return st


def _chain_case(L, oracle, t, chain, op, rtol):
    import test_mapiter as M
    chains = M.CHAINS[5](t.n_tracks) if BIG_CHAINS[chain] is None else BIG_CHAINS[chain](t.n_tracks)
    exp_t = M._expected_tracks(oracle, t, chains)
    mark = len(M._KEEP)
    its = (C.c_void_p * t.n_tracks)(*M._readers(L, t, chains))
    wi = getattr(L, M.REDUCERS[op])(L.newMultiplexer(its, t.n_tracks, b"\x00"))
    got = _blocks_np(L, wi, t.chrom_names)
    st = _pipe_stats(L, wi)
    del M._KEEP[mark:]                                      # (the readers are drained: their arrays may go)
    ec, es, ef, ev = oracle.reduce(exp_t.as_dict(), op)
    assert np.array_equal(got[0], ec) and np.array_equal(got[1], es) and np.array_equal(got[2], ef), (chain, op)
    if rtol == 0.0:
        assert _bits_equal(got[3], ev), (chain, op)
    else:
        a, b = got[3], ev
        assert np.array_equal(np.isnan(a), np.isnan(b)), (chain, op)
        fin = ~np.isnan(b) & np.isfinite(b)
        assert _bits_equal(a[~fin], b[~fin]), (chain, op)
        assert np.all(np.abs(a[fin] - b[fin]) <= rtol * np.maximum(np.abs(b[fin]), 1e-300)), (chain, op)
    return st


@gpu
@pytest.mark.parametrize("n_chrom", [1, 3])
@pytest.mark.parametrize("chain", list(BIG_CHAINS))
def test_gpu_map_chains_over_big_batches(oracle, chain, n_chrom):
    """`sum` and `mean` over 8 float32 tracks of >= 4e5 runs each behind operator chains, default batch sizes: some batch
    holds more than 262 144 input runs -- shown from the pipe's own counters (intervals / batches) -- so the chain kernels'
    block scan carries.  Expectations: test_mapiter._expected_tracks and oracle.reduce; 1e-12 as in test_mapiter, the
    float32-exact chain's `sum` bit for bit."""
    import test_mapiter as M
    from wiggletools_amd import _lib
    L = M._bind(_lib.lib())
    t = _big_tracks(n_chrom)
    per_track = [sum(int(t.seg_off[c * 8 + i + 1] - t.seg_off[c * 8 + i]) for c in range(t.n_chrom)) for i in range(8)]
    assert min(per_track) >= 400_000, per_track
    for op in ("sum", "mean"):
        st = _chain_case(L, oracle, t, chain, op, 0.0 if (chain == "f32-exact" and op == "sum") else 1e-12)
        print("map chain %s, %s, %d chromosome(s): %d input runs in %d batches" % (chain, op, n_chrom, st.intervals, st.batches))
        assert st.intervals > st.batches * WM_CARRY, (st.intervals, st.batches)        # => a batch above 262 144 runs


# =====================================================================================================================
# 4. wt_auc_kernel, wt_pearson_kernel
# =====================================================================================================================
# wt_runs_auc_span: 512 blocks of 256 lanes, grid stride = 131 072 runs.
AUC_STRIDE = 512 * 256


@gpu
@pytest.mark.parametrize("n", [0, 1, AUC_STRIDE - 1, AUC_STRIDE, AUC_STRIDE + 1, 10_000_001])
def test_gpu_auc_and_mean_exact(engine, n):
    """Exact-by-construction lists with NaN runs: auc() is the integer sum and mean() is sum / span of the exact integers,
    bit for bit -- one dropped or doubled run among 10^7 shows."""
    s, f, v, eighths = exact.exact_by_construction(np.random.default_rng(n + 1), n, signed=True, nan_prob=0.02)
    r = _runs(engine, s, f, v)
    span = float((f.astype(np.int64) - s)[~np.isnan(v)].sum())
    auc, mean = r.auc(), r.mean()
    assert auc == eighths / 8.0, (n, auc, eighths / 8.0)
    if n == 0:
        assert np.isnan(mean)
    else:
        assert mean == (eighths / 8.0) / span, (n, mean)
    assert r.auc() == auc


# wt_pearson_impl: 256 blocks of 256 lanes = 65 536 lanes, contiguous slices of ceil(n / 65536) runs.
PEARSON_LANES = 256 * 256


def _tile_tracks(rng, R, gaps, defaults=(0.0, 0.0), xy=None):
    """Two tracks whose Multiplexer tile has exactly R runs.  gaps: holes in the tile, runs where only one track is in play;
    the first track is absent at the very start, the second at the very end.  Values k / 8 (or xy[:, 0], xy[:, 1])."""
    from wiggletools_amd.runlists import RunLists
    L = rng.integers(1, 9, R).astype(np.int64)
    gap = (rng.random(R) < 0.1) * rng.integers(1, 5, R) if gaps else np.zeros(R, np.int64)
    start = 1 + np.cumsum(gap + np.concatenate([[0], L[:-1]]))
    finish = start + L
    p = rng.integers(0, 4, R) if gaps else np.full(R, 2)    # 0: only x, 1: only y, 2, 3: both
    if gaps:
        p[0], p[-1] = 1, (0 if R > 1 else 1)
    kx = rng.integers(0, 800, R)
    x = kx / 8.0 if xy is None else xy[:, 0]
    y = (kx // 2 + rng.integers(0, 400, R)) / 8.0 if xy is None else xy[:, 1]       # (correlated: T_xy is not a near-zero)
    px, py = p != 1, p != 0
    t = RunLists(1, 2, [0, int(px.sum()), int(px.sum() + py.sum())], np.concatenate([start[px], start[py]]),
                 np.concatenate([finish[px], finish[py]]), np.concatenate([x[px], y[py]]), list(defaults))
    return t


def _pearson_check(oracle, engine, t, R, what, exact_sums=True):
    d = t.as_dict()
    c, s, f, vals, ip = oracle.multiplex(d)
    assert len(s) == R, (what, len(s), R)
    em, er = exact.pearson_exact(s, f, vals, ip, t.defaults)
    sm = exact.seq_pearson(s, f, vals, ip, t.defaults)
    ts = engine.TrackSet.from_runlists(t)
    gm, gr = ts.pearson_moments(), ts.pearson()
    ts.close()
    worst = 0.0
    for k, name in enumerate(("n", "Sx", "Sy", "Txx", "Txy", "Tyy")):
        if k < 3 and exact_sums:
            assert gm[k] == em[k], (what, name, gm[k], em[k])          # exact by construction
        else:
            bound = max(4 * rel_err(sm[k], em[k]), REL)
            worst = max(worst, rel_err(gm[k], em[k]))
            assert rel_err(gm[k], em[k]) <= bound, (what, name, gm[k], em[k], sm[k])
    seq_r = oracle.pearson(d)
    print("pearson %s: worst device error in the moments %.3g; correlation exact %.17g device error %.3g (oracle %.3g)"
          % (what, worst, er, rel_err(gr, er), rel_err(seq_r, er)))
    assert rel_err(gr, er) <= max(4 * rel_err(seq_r, er), REL), (what, gr, er, seq_r)
    return gr


@gpu
@pytest.mark.parametrize("R", [1, 2, PEARSON_LANES - 1, PEARSON_LANES, PEARSON_LANES + 1, 1_000_003])
def test_gpu_pearson_slices(oracle, engine, R):
    """Tile run counts around the 65 536 lanes (at 65 537 the slices are 2 runs and the upper lanes empty) and ~1e6, with and
    without gaps, with non-zero defaults, one track absent at the very start and at the very end: n, Sx, Sy bit for bit
    (exact by construction), Txx / Txy / Tyy and the correlation held to max(4 x the sequential update's error, 1e-9)."""
    if R > exact.FRACTION_MAX:
        _need_long_double()
    for gaps, defaults in ((False, (0.0, 0.0)), (True, (0.0, 0.0)), (True, (0.5, -2.0))):
        t = _tile_tracks(np.random.default_rng(R + gaps), R, gaps, defaults)
        _pearson_check(oracle, engine, t, R, "R=%d gaps=%s defaults=%s" % (R, gaps, defaults))


@gpu
def test_gpu_pearson_constant_track_rule(oracle, engine):
    """txx <= n mx^2 1e-14 -> NaN, pinned on both sides: an exactly constant track gives NaN (however long: the slices'
    merges must not invent a variance), a track whose relative variance is 1e-10 a finite value within the bound."""
    R = 70_001
    rng = np.random.default_rng(2)
    y = 40 + 5 * rng.standard_normal(R)
    for const in (3.5, 1000.1, 1e-3):
        for xy in (np.stack([np.full(R, const), y], axis=1), np.stack([y, np.full(R, const)], axis=1)):
            t = _tile_tracks(np.random.default_rng(3), R, False, xy=xy)
            ts = engine.TrackSet.from_runlists(t)
            got = ts.pearson()
            ts.close()
            assert np.isnan(got), (const, got)
    x = 1000.0 * (1 + 1e-5 * rng.standard_normal(R))        # relative variance 1e-10: four decades above the rule
    xy = np.stack([x, 0.5 * (x - 1000.0) * 100 + y], axis=1)
    got = _pearson_check(oracle, engine, _tile_tracks(np.random.default_rng(4), R, False, xy=xy), R, "relative variance 1e-10",
                         exact_sums=False)
    assert np.isfinite(got) and 0 < abs(got) <= 1
