"""What tests/test_compose_model.py (the emulated drop-in library: host sweeps) and tests/test_compose_gpu.py (the product) share:
the drop-in iterators STACKED -- an operator iterator as the child of another, of a statistic, of a writer or of a reducer, as
the reference's grammar builds them (`bin 100 smooth 8 x`, `overlaps mask smooth 8 x`, `sum (smooth 8 a) (smooth 8 b)`).

A producer P delivers doubles that are exact in binary but not in float32 (at least half of them: check_producer).  Every
consumer K is read twice: over the stacked P, and over a popping child that replays read_pops(P) one double at a time -- the
reference's protocol, in which a consumer only ever sees pop().  Two assertions per (P, K), neither with a tolerance:

  (a) replay identity: K(P) equals K(replay of read_pops(P)) bit for bit -- coordinates, values, counts, moments, rows, bytes;
  (b) the model: K's exact model over read_pops(P), bit for bit.  Every value is a dyadic rational well inside 53 bits, so
      every sum is exact in any order.  Two consumers round: the energy integrator (the bound tests/energy_model.py derives)
      and the profile bins whose terms are not multiples of 1/1024 (the bound of profile_model.check_row); both still hold (a).

The source tracks hold runs of mostly one bp, mostly touching, with values k / 8, 2^23 <= k < 2^24, consecutive k of opposite parity: a window of
two adjacent runs sums to an odd number of 25 bits, which no float32 holds (values below 2^20 cannot show this at width 2: the
sum of two 23-bit numbers fits 24 bits), and the sums of 8 and 64 carry 27 and 30 bits."""
import ctypes as C
import os

import numpy as np

import apply_model as AM
import energy_model as EM
import hist_dropin
import hist_model as HM
import profile_dropin
import profile_model as PM
import region_dropin
import region_model as RM
import text_dropin
import text_model as TM
import window_dropin
import window_model as WM

NAMES = ("chr1", "chr2", "chr3")
SHORT = 5                               # positions of the last of three chromosomes: shorter than the widths 8 and 64
# (the Feeder takes a served child in blocks only past the rows its Multiplexer was primed with, about 2000: the two longer
# lengths; the Fraction models and the replay, a Python callback per pop, take 8 to 14 s a case at 20 000 positions)
SHAPES = [(60, 1), (60, 3), (3000, 1), (3000, 3), (8000, 1), (8000, 3)]
MAP_SCALE, MAP_OFFSET = 0, 1            # WTAMD_MAP_*
REDUCERS = ("Sum", "Mean", "Min", "Max", "Median")
NO_DEVICE = ("WTAMD_NO_DEVICE_WINDOW", "WTAMD_NO_DEVICE_REGION", "WTAMD_NO_DEVICE_COVERAGE", "WTAMD_NO_DEVICE_HIST", "WTAMD_NO_DEVICE_ENERGY",
             "WTAMD_NO_DEVICE_TEXT", "WTAMD_NO_DEVICE_APPLY", "WTAMD_NO_DEVICE_PROFILE")


class Doors:
    """The ctypes drivers of the doors' own test modules over one library: an iterator is an address, whichever built it."""

    def __init__(self, path):
        self.win, self.reg, self.hist = window_dropin.DropIn(path), region_dropin.DropIn(path), hist_dropin.DropIn(path)
        self.text, self.prof = text_dropin.DropIn(path), profile_dropin.DropIn(path)        # (and the energy integrator; and apply)
        L = self.L = self.win.L
        L.wtamd_MapIterator.restype = C.c_void_p
        L.wtamd_MapIterator.argtypes = [C.c_void_p, C.c_int, C.c_double]
        for op in REDUCERS:
            getattr(L, op + "Reduction").restype = C.c_void_p
            getattr(L, op + "Reduction").argtypes = [C.c_void_p]
        self.reader, self.popping, self.fields = self.win.reader, self.win.popping, self.win.fields
        self.read_pops, self.read_blocks, self.seek = self.win.read_pops, self.win.read_blocks, self.win.seek

    def map(self, child, op, param):
        return self.L.wtamd_MapIterator(child, op, float(param))

    def reduce(self, op, kids):
        arr = (C.c_void_p * len(kids))(*kids)
        self.win.keep.append(arr)
        return getattr(self.L, op + "Reduction")(self.L.newMultiplexer(arr, len(kids), b"\x00"))


# ---------------------------------------------------------------------------------------------------------------------
# Shapes
# ---------------------------------------------------------------------------------------------------------------------
class Shape:
    """n_chrom chromosomes, the first of `length` positions, the second of a third of it, the last of three of SHORT; four
    source tracks of disjoint runs (values exact in float32), an overlapping track, and an overlapping mask."""

    def __init__(self, length, n_chrom, seed=5):
        rng = np.random.default_rng(seed + length + n_chrom)
        self.length, self.names = length, list(NAMES[:n_chrom])
        self.lengths = [length, max(length // 3, 9), SHORT][:n_chrom] if n_chrom > 1 else [length]
        if n_chrom == 3:
            self.lengths[2] = SHORT
        self.tracks = [[self._runs(rng, n) for n in self.lengths] for _ in range(4)]
        self.mask = [self._mask(rng, n) for n in self.lengths]
        self.over = [(np.repeat(s, 2), np.stack([f, f + 1 + np.arange(len(f)) % 3]).T.ravel()) for s, f, _ in self.tracks[0]]

    @staticmethod
    def _runs(rng, length):
        s, f, pos = [], [], 1 + int(rng.integers(0, 2))
        while pos <= length:
            ln, gap = int(rng.choice((1,) * 20 + (2, 3))), int(rng.choice((0,) * 20 + (1, 3)))
            if length >= 3000 and pos < length // 2 <= pos + ln + gap:
                gap = 70                # one gap wider than every window: smooth reads zeros across it
            s.append(pos); f.append(min(pos + ln, length + 1))
            pos = f[-1] + gap
        n = len(s)
        k = (1 << 23) + 2 * rng.integers(0, 1 << 22, n) + (np.arange(n) & 1)
        return np.array(s, np.int32), np.array(f, np.int32), k / 8.0

    @staticmethod
    def _mask(rng, length):
        s = np.sort(rng.integers(1, length + 1, max(length // 12, 2))).astype(np.int32)
        return s, (s + rng.integers(1, 9, len(s))).astype(np.int32)

    def source(self, D, i):
        return D.reader(self.names, *_flat(self.tracks[i]), overlapping=False)

    def mask_reader(self, D):
        seg, s, f = _flat2(self.mask)
        return D.reader(self.names, seg, s, f, np.ones(len(s), np.float32), overlapping=True)

    def overlapping(self, D):
        seg, s, f = _flat2(self.over)
        return D.reader(self.names, seg, s, f, np.ones(len(s), np.float32), overlapping=True)


def _flat(chroms):
    seg = np.concatenate([[0], np.cumsum([len(c[0]) for c in chroms])]).astype(np.int64)
    return seg, np.concatenate([c[0] for c in chroms]), np.concatenate([c[1] for c in chroms]), np.concatenate([c[2] for c in chroms])


def _flat2(chroms):
    return _flat([(s, f, np.ones(len(s))) for s, f in chroms])[:3]


def _coords_reader(D, names, chroms):
    """An overlapping reader (a BED reader: only coordinates matter) over the chromosomes that have intervals."""
    has = [k for k in range(len(names)) if len(chroms[k][0])]
    seg, s, f = _flat2([chroms[k] for k in has] or [(np.zeros(0, np.int32),) * 2])
    return D.reader([names[k] for k in has] or names[:1], seg, s, f, np.ones(len(s), np.float32), overlapping=True)


_shapes = {}


def shape(length, n_chrom):
    if (length, n_chrom) not in _shapes:
        _shapes[(length, n_chrom)] = Shape(length, n_chrom)
    return _shapes[(length, n_chrom)]


# ---------------------------------------------------------------------------------------------------------------------
# Producers: (D, shape, i) -> a fresh stacked iterator over source track i
# ---------------------------------------------------------------------------------------------------------------------
def _smooth(w):
    return lambda D, S, i: D.win.window("smooth", S.source(D, i), w)


def _region_of_smooth(op):
    return lambda D, S, i: D.reg.region(op, _smooth(8)(D, S, i), S.mask_reader(D))


def _nearest(D, S, i):
    """Two source runs and one far mask per chromosome: distances 2^25 + 3 and 2^24 + 1, odd and above 2^24."""
    m = (1 << 25) + 20 + i
    s, f = np.array([17 + i, m - (1 << 24) - 1], np.int32), np.array([18 + i, m - (1 << 24)], np.int32)
    n = len(S.names)
    seg = np.arange(n + 1, dtype=np.int64)
    src = D.reader(S.names, 2 * seg, np.tile(s, n), np.tile(f, n), np.ones(2 * n, np.float32), overlapping=False)
    mask = D.reader(S.names, seg, np.full(n, m, np.int32), np.full(n, m + 5, np.int32), np.ones(n, np.float32), overlapping=True)
    return D.reg.region("nearest", src, mask)


def _mean4(D, S, i):
    return D.reduce("Mean", [_smooth(w)(D, S, (i + j) % 4) for j, w in enumerate((2, 8, 64, 8))])


PRODUCERS = {
    "smooth2": _smooth(2), "smooth8": _smooth(8), "smooth64": _smooth(64),
    "bin_of_smooth": lambda D, S, i: D.win.window("bin", _smooth(8)(D, S, i), 10),
    "trim_of_smooth": _region_of_smooth("trim"), "overlaps_of_smooth": _region_of_smooth("overlaps"),
    "noverlaps_of_smooth": _region_of_smooth("noverlaps"),
    "nearest_far": _nearest,
    "scale_of_smooth": lambda D, S, i: D.map(_smooth(8)(D, S, i), MAP_SCALE, 1.0 / 64),
    "mean_of_four": _mean4,             # a reducer of this library: not served through the bulk door of a run list
    "coverage_control": lambda D, S, i: D.win.coverage(S.overlapping(D)),      # integers: a control that must not change
}
CONTROLS = ("coverage_control",)
# (nearest_far does not depend on the length: it runs at the shortest one)
CASES = [(p, n, c) for p in sorted(PRODUCERS) for n, c in SHAPES if p != "nearest_far" or n == SHAPES[0][0]]
NO_BLOCK_DOOR = ("scale_of_smooth",)    # wtamd_iterator_next_block serves run lists and reducers, not operator handles
# (smooth reads a gap inside a chromosome as zeros, position by position: 2^24 rows between the two runs of nearest_far)
NOT_RUN = {("nearest_far", "smooth3")}


def check_producer(rows, name):
    """The condition of the test: at least half of a non-control producer's popped values are not float32-exact, and every
    one is a dyadic rational of at most 38 bits (so that the sums over 20 000 positions stay exact)."""
    v = np.array([r[3] for r in rows], np.float64)
    assert len(v) and np.isfinite(v).all(), name
    assert np.array_equal(np.ldexp(v, 12), np.rint(np.ldexp(v, 12))) and np.abs(v).max() < 2.0 ** 26, name
    inexact = int((v.astype(np.float32).astype(np.float64) != v).sum())
    if name in CONTROLS:
        assert inexact == 0, name
    else:
        assert 2 * inexact >= len(v), (name, inexact, len(v))


# ---------------------------------------------------------------------------------------------------------------------
# What a child delivered, as the models take it
# ---------------------------------------------------------------------------------------------------------------------
class Pops:
    """read_pops() of a child over the chromosomes `names`, and the child's default_value."""

    def __init__(self, rows, names, default):
        self.rows, self.names, self.default = rows, list(names), float(default)
        self.chroms = [(np.array([r[1] for r in rows if r[0] == n], np.int32), np.array([r[2] for r in rows if r[0] == n], np.int32),
                        np.array([r[3] for r in rows if r[0] == n], np.float64)) for n in self.names]
        self.seg, self.s, self.f, self.v = _flat(self.chroms)

    def replay(self, D):
        return D.popping(self.names, self.seg, self.s, self.f, self.v, default=self.default)

    def regions(self):
        """Up to eight regions per chromosome cut from the rows themselves: whole rows, parts of rows, overlapping ones."""
        out = []
        for s, f, _ in self.chroms:
            n = len(s)
            idx = sorted(set(int(x) for x in np.linspace(0, max(n - 1, 0), 8))) if n else []
            rs = [int(s[a]) + (k % 2) * (int(f[a]) - int(s[a]) > 1) for k, a in enumerate(idx)]
            rf = [min(int(f[min(a + (3 * k + 1) * max(n // 40, 1), n - 1)]), x + 4096) for (k, a), x in zip(enumerate(idx), rs)]
            out.append((np.array(rs, np.int32), np.array(rf, np.int32)))
        return out

    def mask(self):
        """An overlapping mask cut from the rows: every fifth row with its successor, shifted by one position."""
        out = []
        for s, f, _ in self.chroms:
            a = np.arange(0, len(s), 5)
            b = np.minimum(a + 1, len(s) - 1)
            out.append((s[a] + 1, np.maximum(f[b], s[a] + 2).astype(np.int32)))
        return out


def bits(rows):
    """Rows as a tuple that compares bit for bit (any NaN equal to any NaN)."""
    return [(r[0], r[1], r[2], "nan" if r[3] != r[3] else float(r[3]).hex()) for r in rows]


def _hex(a):
    return ["nan" if x != x else float(x).hex() for x in np.asarray(a, np.float64).ravel()]


# ---------------------------------------------------------------------------------------------------------------------
# Consumers: run(D, S, kid) -> a result that compares with ==, kid(i) a fresh child (stacked or replayed) over track i;
# model(D, S, pops, got): asserts the exact model over pops(i) = what P over track i delivered
# ---------------------------------------------------------------------------------------------------------------------
class Window:
    def __init__(self, op, w):
        self.op, self.w, self.name = op, w, "%s%d" % (op, w)

    def run(self, D, S, kid):
        return bits(D.read_pops(D.win.window(self.op, kid(0), self.w)))

    def expected(self, p):
        return bits(window_dropin._model_rows(self.op, WM.Case(p.chroms), p.names, self.w, p.default))

    def model(self, D, S, pops, got):
        assert got == self.expected(pops(0)), self.name


class Region:
    def __init__(self, op, as_mask):
        self.op, self.as_mask, self.name = op, as_mask, "%s_%s" % (op, "as_mask" if as_mask else "as_source")

    def run(self, D, S, kid):
        if self.as_mask:
            return bits(D.read_pops(D.reg.region(self.op, S.source(D, 1), kid(0))))
        return bits(D.read_pops(D.reg.region(self.op, kid(0), _coords_reader(D, self._pops.names, self._pops.mask()))))

    def prepare(self, pops):
        self._pops = pops(0)

    def model(self, D, S, pops, got):
        p = pops(0)             # (its chromosomes are the shape's, some of them perhaps empty)
        src, mask = (_flat(S.tracks[1]), (p.seg, p.s, p.f)) if self.as_mask else ((p.seg, p.s, p.f, p.v), _flat2(p.mask()))
        assert got == bits(region_dropin.expected_rows(self.op, p.names, *src, *mask)), self.name


class Histogram:
    name = "histogram20"

    def run(self, D, S, kid):
        r2, m, txt, ntxt = D.hist.histogram([kid(0)], 20)
        return _hex(r2), _hex(m), txt, ntxt

    def model(self, D, S, pops, got):
        p = pops(0)
        rng, m = HM.histogram(HM.Lists.from_rows([(p.s, p.f, p.v)]), 20)
        assert got == (_hex(rng), _hex(m), HM.text(rng, m), HM.text(rng, HM.normalize(m))), self.name


class Energy:
    """(The device door and the host sweep of the energy integrator each keep the bound, not each other's bits -- INTEGRATION.md:
    "its own error bound, not bit for bit" -- so the host's re-read is held to the bound of (b) too.)"""
    name, lam, host_bits = "energy7", 7, False

    def run(self, D, S, kid):
        return _hex(D.text.integrate(kid(0), self.lam)[:3])

    def model(self, D, S, pops, got):
        p = pops(0)
        L = EM.Lists(p.seg, p.s, p.f, p.v)
        re_im = np.array([[float.fromhex(x) for x in got[:2]]])
        EM.check_close(re_im, EM.exact(L, [self.lam]), len(L.s), EM.weight(L), self.name)
        assert got[2] == _hex(EM.energy(re_im))[0], self.name


class Apply:
    name, stats = "apply", ("AUC", "meanI", "maxI", "minI")

    def prepare(self, pops):
        self._pops = pops(0)

    def _regions(self, D):
        return _coords_reader(D, self._pops.names, self._pops.regions())

    def run(self, D, S, kid):
        out = []
        for strict in (True, False):
            rows = D.prof.read_mux(D.prof.apply(self._regions(D), self.stats, kid(0), strict))
            out.append([(r[0], r[1], r[2], _hex(r[3])) for r in rows])
        return out

    def model(self, D, S, pops, got):
        p = pops(0)
        for rows, strict in zip(got, (True, False)):
            exp = []
            for n, (s, f, v), (rs, rf) in zip(p.names, p.chroms, p.regions()):
                for a, b in zip(rs, rf):
                    m = AM.region_moments(s, f, v, int(a), int(b), p.default, strict)
                    exp.append((n, int(a), int(b), _hex([AM.finish(m, q) for q in self.stats])))
            assert rows == exp, (self.name, strict)


class Profile(Apply):
    name, W = "profile", 8

    def run(self, D, S, kid):
        rows = D.prof.read_mux(D.prof.profile(self._regions(D), self.W, kid(0)))
        return [(r[0], r[1], r[2], _hex(r[3])) for r in rows]

    def model(self, D, S, pops, got):
        p = pops(0)
        k = 0
        for n, (s, f, v), (rs, rf) in zip(p.names, p.chroms, p.regions()):
            for a, b in zip(rs, rf):
                assert got[k][:3] == (n, int(a), int(b)), self.name
                PM.check_row([float.fromhex(x) if x != "nan" else np.nan for x in got[k][3]], PM.closed(s, f, v, int(a), int(b), self.W, p.default), (self.name, k))
                k += 1
        assert k == len(got), self.name


class Tee:
    def __init__(self, bed, tmp):
        self.bed, self.name, self.path = bed, "tee_bedgraph" if bed else "tee_wig", os.path.join(str(tmp), "compose.txt")

    def run(self, D, S, kid):
        wi, fp = D.text.tee(kid(0), self.path, self.bed)
        rows = D.read_pops(wi)
        return bits(rows), D.text.written(fp, self.path)

    def model(self, D, S, pops, got):
        p = pops(0)
        L = TM.Lists(p.names, p.seg, p.s, p.f, p.v)
        want = L if self.bed else TM.compress(L)
        assert got[1] == TM.text(want, TM.BEDGRAPH if self.bed else 0)[0], self.name
        assert got[0] == bits(text_dropin.rows_of(want)), self.name


class Reducer:
    """newMultiplexer + a reducer of this library over n children, each optionally under a fused chain scale 1/64, offset 1/2."""

    def __init__(self, op, n, chain):
        self.op, self.n, self.chain, self.name = op, n, chain, "%s%d%s" % (op.lower(), n, "_chained" if chain else "")

    def _kid(self, D, kid, i):
        return D.map(D.map(kid(i), MAP_SCALE, 1.0 / 64), MAP_OFFSET, 0.5) if self.chain else kid(i)

    def run(self, D, S, kid):
        return bits(D.read_blocks(D.reduce(self.op, [self._kid(D, kid, i) for i in range(self.n)])))

    def model(self, D, S, pops, got):
        ps = [pops(i) for i in range(self.n)]
        names = sorted(set(n for p in ps for n in p.names))
        f = (lambda v: v / 64 + 0.5) if self.chain else (lambda v: v)
        seg, s, e, v = [0], [], [], []
        for n in names:
            for p in ps:
                cs, cf, cv = p.chroms[p.names.index(n)] if n in p.names else ([], [], [])
                s += list(cs); e += list(cf); v += list(f(np.asarray(cv, np.float64)))
                seg.append(len(s))
        t = dict(n_chrom=len(names), n_tracks=self.n, seg_off=np.array(seg, np.int64), start=np.array(s, np.int32), finish=np.array(e, np.int32),
                 value=np.array(v, np.float64), defaults=np.array([float(f(np.float64(p.default))) for p in ps]))
        ec, es, ef, ev = self.oracle.reduce(t, self.op.lower())[:4]
        assert got == bits([(names[c], int(a), int(b), float(x)) for c, a, b, x in zip(ec, es, ef, ev)]), self.name


class Blocks:
    """wtamd_iterator_next_block over P itself: the replay is the list of pops."""

    def __init__(self, pops_between):
        self.k, self.name = pops_between, "next_block_pops%d" % pops_between

    def run(self, D, S, kid):
        return bits(D.read_blocks(kid(0), pops_between=self.k))

    def model(self, D, S, pops, got):
        assert got == bits(pops(0).rows), self.name


def consumers(tmp, oracle):
    out = [Window("bin", 10), Window("smooth", 3)]
    out += [Region(op, False) for op in sorted(RM.OPS)] + [Region(op, True) for op in sorted(RM.OPS)]
    out += [Histogram(), Energy(), Apply(), Profile(), Tee(False, tmp), Tee(True, tmp)]
    out += [Reducer(op, n, chain) for chain in (False, True) for op in REDUCERS for n in (2, 4)]
    out += [Blocks(0), Blocks(2)]
    for k in out:
        k.oracle = oracle
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The checks
# ---------------------------------------------------------------------------------------------------------------------
def _pops_of(D, S, make):
    cache = {}

    def pops(i):
        if i not in cache:
            wi = make(D, S, i)
            cache[i] = Pops(D.read_pops(wi), S.names, D.fields(wi).default_value)
        return cache[i]
    return pops


def check_stack(D, oracle, tmp, producer, length, n_chrom, setenv=None, only=None):
    """Every consumer over one producer at one shape: (a) and (b).  setenv(name, value): given by the product's test, which
    reads every stack once more with the matching WTAMD_NO_DEVICE_*=1 and expects the same bits.  Returns the names of the
    consumers that failed with what they said (so that one wrong consumer does not hide the others)."""
    S, make = shape(length, n_chrom), PRODUCERS[producer]
    pops = _pops_of(D, S, make)
    check_producer(pops(0).rows, producer)
    failed = []
    for K in consumers(tmp, oracle):
        if (only is not None and K.name not in only) or (isinstance(K, Blocks) and producer in NO_BLOCK_DOOR) or (producer, K.name) in NOT_RUN:
            continue
        if hasattr(K, "prepare"):
            K.prepare(pops)
        try:
            got = K.run(D, S, lambda i: make(D, S, i))
            if isinstance(K, Blocks):
                replay = bits(pops(0).rows)
            else:
                replay = K.run(D, S, lambda i: pops(i).replay(D))
            assert got == replay, (K.name, "the stacked child against the replay of its pops")
            K.model(D, S, pops, got)
            if setenv:
                for var in NO_DEVICE:
                    setenv(var, "1")
                try:
                    host = K.run(D, S, lambda i: make(D, S, i))
                finally:
                    for var in NO_DEVICE:
                        setenv(var, "0")
                if getattr(K, "host_bits", True):
                    assert host == got, (K.name, "host sweeps against the device doors")
                else:
                    K.model(D, S, pops, host)
        except AssertionError as e:
            failed.append((K.name, str(e)[:300]))
    return failed


SEEKERS = ("bin", "smooth", "overlaps")


def check_seek(D, producer, length, n_chrom):
    """K in bin, smooth, overlaps: pop once, seek(K(P)); the result is K's model over what a fresh P delivers after the same
    seek (and, for overlaps, what a fresh mask delivers after it)."""
    S, make = shape(length, n_chrom), PRODUCERS[producer]
    rows = D.read_pops(make(D, S, 0))
    g = S.names[-2] if n_chrom > 1 else S.names[0]
    on = [r for r in rows if r[0] == g]
    lo, hi = on[len(on) // 5][1] + 1, on[4 * len(on) // 5][2] - 1
    if hi <= lo:
        return 0
    fresh = make(D, S, 0)
    default = D.fields(fresh).default_value
    D.seek(fresh, g, lo, hi)
    p = Pops(D.read_pops(fresh), S.names, default)
    for k in SEEKERS:
        if (producer, k + "3") in NOT_RUN:
            continue
        if k == "overlaps":
            wi = D.reg.region(k, make(D, S, 0), S.mask_reader(D))
            m = S.mask_reader(D)
            D.seek(m, g, lo, hi)
            mp = Pops(D.read_pops(m), S.names, 0.0)
            exp = region_dropin.expected_rows(k, p.names, p.seg, p.s, p.f, p.v, mp.seg, mp.s, mp.f)
        else:
            w = 10 if k == "bin" else 3
            wi = D.win.window(k, make(D, S, 0), w)
            exp = window_dropin._model_rows(k, WM.Case(p.chroms), p.names, w, default)
        D.L.pop(wi)
        D.seek(wi, g, lo, hi)
        assert bits(D.read_pops(wi)) == bits(exp), (producer, k, "seek", g, lo, hi)
    return len(SEEKERS)


# ---------------------------------------------------------------------------------------------------------------------
# The recorded stacks (tests/golden/make_compose_golden.py): a stack is a postfix program of [op, argument] steps over
# numbered array children -- ["src", i] pushes track i, ["mask", 0] the overlapping mask, ["smooth" | "bin", width] and
# ["scale", factor] wrap the top, the four region operators take (source, mask) off the stack, ["sum" | "mean", n] take n
# ---------------------------------------------------------------------------------------------------------------------
STACKS = {
    "bin4_of_smooth8": [["src", 0], ["smooth", 8], ["bin", 4]],
    "bin10_of_smooth2": [["src", 0], ["smooth", 2], ["bin", 10]],
    "smooth8_of_bin4": [["src", 0], ["bin", 4], ["smooth", 8]],
    "smooth3_of_bin10": [["src", 1], ["bin", 10], ["smooth", 3]],
    "overlaps_of_smooth8": [["src", 0], ["smooth", 8], ["mask", 0], ["overlaps", 0]],
    "noverlaps_of_smooth8": [["src", 1], ["smooth", 8], ["mask", 0], ["noverlaps", 0]],
    "trim_of_bin10": [["src", 0], ["bin", 10], ["mask", 0], ["trim", 0]],
    "trim_of_smooth2": [["src", 1], ["smooth", 2], ["mask", 0], ["trim", 0]],
    "nearest_beyond_2p24": [["src", 3], ["mask", 1], ["nearest", 0]],
    "bin10_of_nearest_beyond_2p24": [["src", 3], ["mask", 1], ["nearest", 0], ["bin", 10]],
    "sum_of_two_smooth8": [["src", 0], ["smooth", 8], ["src", 1], ["smooth", 8], ["sum", 2]],
    "mean_of_smooth8_and_smooth2": [["src", 0], ["smooth", 8], ["src", 2], ["smooth", 2], ["mean", 2]],
    "sum_of_two_scaled_smooth8": [["src", 0], ["smooth", 8], ["scale", 1.0 / 64], ["src", 1], ["smooth", 8], ["scale", 1.0 / 64], ["sum", 2]],
    "mean_of_three_stacks": [["src", 0], ["smooth", 8], ["bin", 4], ["src", 1], ["smooth", 8], ["mask", 0], ["trim", 0], ["src", 2], ["mean", 3]],
}
REGION_OPS = ("overlaps", "noverlaps", "trim", "nearest")


def golden_lists(length, n_chrom):
    """What the recorded stacks run over: (names, tracks 0..2 from the Shape, track 3 = the two far runs of nearest_far, masks
    0 = the Shape's, 1 = the far one), every list per chromosome of `names`."""
    S = Shape(length, n_chrom, seed=41)
    m = (1 << 25) + 20
    far = [(np.array([17, m - (1 << 24) - 1], np.int32), np.array([18, m - (1 << 24)], np.int32), np.array([1.0, 1.0]))] * n_chrom
    far_mask = [(np.array([m], np.int32), np.array([m + 5], np.int32))] * n_chrom
    return S.names, S.tracks[:3] + [far], [S.mask, far_mask]


def fixture_lists(c):
    names = c["chrom_names"]
    tracks = [[(np.array(s, np.int32), np.array(f, np.int32), np.array(v, np.float64)) for s, f, v in t] for t in c["tracks"]]
    masks = [[(np.array(s, np.int32), np.array(f, np.int32)) for s, f in m] for m in c["masks"]]
    return names, tracks, masks


def build_stack(D, prog, names, tracks, masks):
    """The program as stacked drop-in iterators."""
    st = []
    for op, arg in prog:
        if op == "src":
            st.append(D.reader(names, *_flat(tracks[arg]), overlapping=False))
        elif op == "mask":
            st.append(_coords_reader(D, names, masks[arg]))
        elif op in ("smooth", "bin"):
            st.append(D.win.window(op, st.pop(), arg))
        elif op == "scale":
            st.append(D.map(st.pop(), MAP_SCALE, arg))
        elif op in REGION_OPS:
            mask, src = st.pop(), st.pop()
            st.append(D.reg.region(op, src, mask))
        else:
            kids = [st.pop() for _ in range(arg)][::-1]
            st.append(D.reduce(op.capitalize(), kids))
    assert len(st) == 1
    return st[0]


def model_stack(prog, names, tracks, masks, oracle):
    """The program through the composed models: [(chrom, start, finish, value)].  Every default is 0."""
    def rows_to_chroms(rows):
        return Pops(rows, names, 0.0).chroms
    st = []
    for op, arg in prog:
        if op == "src":
            st.append(tracks[arg])
        elif op == "mask":
            st.append(masks[arg])
        elif op in ("smooth", "bin"):
            st.append(rows_to_chroms(window_dropin._model_rows(op, WM.Case(st.pop()), names, arg, 0.0)))
        elif op == "scale":
            st.append([(s, f, v * arg) for s, f, v in st.pop()])
        elif op in REGION_OPS:
            mask, src = st.pop(), st.pop()
            st.append(rows_to_chroms(region_dropin.expected_rows(op, names, *_flat(src), *_flat2(mask))))
        else:
            kids = [st.pop() for _ in range(arg)][::-1]
            seg, s, e, v = [0], [], [], []
            for g in range(len(names)):
                for k in kids:
                    s += list(k[g][0]); e += list(k[g][1]); v += list(k[g][2])
                    seg.append(len(s))
            t = dict(n_chrom=len(names), n_tracks=arg, seg_off=np.array(seg, np.int64), start=np.array(s, np.int32), finish=np.array(e, np.int32),
                     value=np.array(v, np.float64), defaults=np.zeros(arg))
            ec, es, ef, ev = oracle.reduce(t, op)[:4]
            st.append(rows_to_chroms([(names[c], int(a), int(b), float(x)) for c, a, b, x in zip(ec, es, ef, ev)]))
    assert len(st) == 1
    return [(n, int(a), int(b), float(x)) for n, (s, f, v) in zip(names, st[0]) for a, b, x in zip(s, f, v)]


def load_fixtures():
    import json
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compose_fixtures.json")) as fh:
        return json.load(fh)["cases"]


def check_fixtures(D, oracle, setenv=None):
    """Every recorded stack through the stacked drop-in iterators, by pop() (and by blocks where the top is a run list or a
    reducer): the reference's recorded doubles, bit for bit; and the composed models give them too."""
    n_inexact = 0
    for c in load_fixtures():
        names, tracks, masks = fixture_lists(c)
        for name, rec in c["stacks"].items():
            prog = rec["program"]
            want = bits([(names[r[0]], r[1], r[2], float(r[3])) for r in rec["rows"]])
            v = np.array([r[3] for r in rec["rows"]], np.float64)
            n_inexact += int((v.astype(np.float32).astype(np.float64) != v).sum())
            assert bits(model_stack(prog, names, tracks, masks, oracle)) == want, (c["name"], name, "model")
            for no_device in (("0", "1") if setenv else ("0",)):
                for var in NO_DEVICE if setenv else ():
                    setenv(var, no_device)
                assert bits(D.read_pops(build_stack(D, prog, names, tracks, masks))) == want, (c["name"], name, "pops", no_device)
                if prog[-1][0] != "scale":
                    assert bits(D.read_blocks(build_stack(D, prog, names, tracks, masks), pops_between=2)) == want, (c["name"], name, "blocks", no_device)
    assert n_inexact >= 1000, n_inexact


def check_feeder_routes(D, oracle, tmp, setenv, delenv):
    """The Feeder's two routes over served children whose values are no float32: the serial one (the default for fewer than 16
    children, here also forced with two drain threads, which a bulk child of this library rules out) and the pooled one (two
    drain threads, every child popped: WTAMD_NO_BULK)."""
    K = ("sum4", "median4", "sum4_chained")
    for env in ({"WTAMD_DRAIN_THREADS": "2"}, {"WTAMD_DRAIN_THREADS": "2", "WTAMD_NO_BULK": "1"}, {"WTAMD_NO_BULK": "1"}):
        for k, x in env.items():
            setenv(k, x)
        try:
            failed = check_stack(D, oracle, tmp, "smooth8", 3000, 1, only=K)
        finally:
            for k in env:
                delenv(k)
        assert not failed, (env, failed)
