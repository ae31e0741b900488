"""The rule of wtamd_runs_energy (include/wiggletools_amd.h, csrc/wt_energy.h): its exact value by mpmath (used by the generator
tests/golden/make_energy_golden.py only; every test reads the recorded values), the error bounds, the recorded fixtures
(tests/golden/energy_fixtures.json: the compiled reference's EnergyIntegrator) and seam values
(tests/golden/energy_seams.json), ctypes drivers of the emulated passes and the host sweep (tests/energy_emu.cpp), and the seam
cases whose sizes come from the header's constants -- shared by tests/test_energy_model.py, test_energy_emu.py,
test_energy_gpu.py, energy_dropin.py and the generator."""
import ctypes as C
import json
import math
import os
import re

import numpy as np

from model_common import _num, bits, same_bits  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "wiggletools_amd", "csrc")
HEADER = os.path.join(CSRC, "wt_energy.h")
MAX_COORD = 2147483647 - 65536                  # WTAMD_MAX_COORD
DOOR_C = 48                                     # the constant of the door's bound (DESIGN.md counts 31 for the kernel as written)


def constants():
    """The WEN_* values of csrc/wt_energy.h: {"BLOCK", "RUNS_PER_LANE", "SHARE", "BATCH", "KCHUNK", "MAX_WAVELENGTHS"}."""
    txt = open(HEADER).read()
    num = lambda k: int(re.search(r"#define WEN_%s (\d+)\b" % k, txt).group(1))      # noqa: E731
    assert re.search(r"#define WEN_BLOCK WCV_BLOCK\b", txt) and re.search(r"#define WEN_SHARE \(WEN_BLOCK \* WEN_RUNS_PER_LANE\)", txt)
    block = int(re.search(r"#define WCV_BLOCK (\d+)", open(os.path.join(CSRC, "wt_cover.h")).read()).group(1))
    c = {k: num(k) for k in ("RUNS_PER_LANE", "BATCH", "KCHUNK", "MAX_WAVELENGTHS")}
    c["BLOCK"] = block
    c["SHARE"] = block * c["RUNS_PER_LANE"]
    return c


class Lists:
    """Run lists as the door takes them: seg (n_seg + 1 offsets), s / f (int32), v (float64)."""

    def __init__(self, seg, s, f, v):
        self.seg = np.ascontiguousarray(seg, np.int64)
        self.s, self.f = np.ascontiguousarray(s, np.int32), np.ascontiguousarray(f, np.int32)
        self.v = np.ascontiguousarray(v, np.float64)
        assert self.seg[0] == 0 and self.seg[-1] == len(self.s) == len(self.f) == len(self.v)

    @classmethod
    def from_segments(cls, segs):
        """segs = [(start, finish, value)] per segment."""
        seg = np.concatenate([[0], np.cumsum([len(r[0]) for r in segs])])
        cat = lambda k, t: np.concatenate([np.asarray(r[k], t) for r in segs] + [np.zeros(0, t)])      # noqa: E731
        return cls(seg, cat(0, np.int32), cat(1, np.int32), cat(2, np.float64))

    @property
    def n_seg(self):
        return len(self.seg) - 1

    def segments(self):
        return [(self.s[a:b], self.f[a:b], self.v[a:b]) for a, b in zip(self.seg[:-1], self.seg[1:])]

    def part(self, a, b):
        """The runs [a, b) with the segments cut accordingly (segments left without a run stay, empty)."""
        return Lists(np.clip(self.seg, a, b) - a, self.s[a:b], self.f[a:b], self.v[a:b])

    def segment(self, g):
        """Segment g alone."""
        a, b = int(self.seg[g]), int(self.seg[g + 1])
        return Lists([0, b - a], self.s[a:b], self.f[a:b], self.v[a:b])

    def as_f32(self):
        return Lists(self.seg, self.s, self.f, self.v.astype(np.float32).astype(np.float64))


def bases(L, seg_base=None):
    """([base per segment], end_base): seg_base, or the reference's rule from 0 -- a segment's base is the sum of the last
    finishes of the non-empty segments before it.  end_base: the base a following segment would get."""
    out, run = [], 0
    end = int(seg_base[-1]) if seg_base is not None and L.n_seg else 0
    for g in range(L.n_seg):
        b = int(seg_base[g]) if seg_base is not None else run
        out.append(b)
        if L.seg[g + 1] > L.seg[g]:
            end = run = b + int(L.f[L.seg[g + 1] - 1])
    return out, end


def weight(L):
    """S = sum |v| L by math.fsum (inf / NaN values: as they come)."""
    return math.fsum(abs(float(v)) * (int(f) - int(s)) for s, f, v in zip(L.s, L.f, L.v))


def exact(L, wavelengths, seg_base=None):
    """The rule evaluated with mpmath at 60 digits, rounded once to double: an array (n_wavelengths, 2) of (real, im).  NaN
    everywhere when a value is NaN or infinite."""
    import mpmath
    out = np.full((len(wavelengths), 2), np.nan)
    if not np.isfinite(L.v).all():
        return out
    base, _ = bases(L, seg_base)
    pos = np.repeat(np.array(base, dtype=object), np.diff(L.seg)) if len(L.s) else []
    with mpmath.workdps(60):
        for k, lam in enumerate(int(x) for x in wavelengths):
            re_, im_ = mpmath.mpf(0), mpmath.mpf(0)
            inv = mpmath.mpf(1) if lam == 1 else 1 / mpmath.sinpi(mpmath.mpf(1) / lam)
            qs = {}
            for i in range(len(L.s)):
                a, ln, v = int(pos[i]) + int(L.s[i]), int(L.f[i]) - int(L.s[i]), mpmath.mpf(float(L.v[i]))
                if lam == 1:
                    re_ += v * ln
                    continue
                m, q = (2 * a + ln - 1) % (2 * lam), ln % (2 * lam)
                if q not in qs:
                    qs[q] = mpmath.sinpi(mpmath.mpf(q) / lam) * inv
                x = mpmath.mpf(m) / lam
                re_ += v * qs[q] * mpmath.cospi(x)
                im_ -= v * qs[q] * mpmath.sinpi(x)
            out[k] = float(re_), float(im_)
    return out


def door_bound(n, S, c=DOOR_C):
    """|x - x*| <= 2^-53 (c + n) S for real and im separately."""
    return 2.0 ** -53 * (c + n) * S


def energy(reim):
    reim = np.asarray(reim, np.float64).reshape(-1, 2)
    return reim[:, 0] * reim[:, 0] + reim[:, 1] * reim[:, 1]


def energy_bound(star, t):
    """|E - E*| <= 2 (|re*| + |im*|) t + 2 t^2."""
    star = np.asarray(star, np.float64).reshape(-1, 2)
    return 2 * (np.abs(star[:, 0]) + np.abs(star[:, 1])) * t + 2 * t * t


def check_close(got, star, n, S, what, c=DOOR_C):
    """got against the exact (n_wavelengths, 2): NaN where the model says NaN, exactly; otherwise inside the bound, and the
    energies inside theirs."""
    got, star = np.asarray(got, np.float64).reshape(-1, 2), np.asarray(star, np.float64).reshape(-1, 2)
    assert got.shape == star.shape, (what, got.shape, star.shape)
    if np.isnan(star).any():
        assert np.isnan(star).all() and np.isnan(got).all(), (what, got)
        return
    t = door_bound(n, S, c)
    err = np.abs(got - star)
    assert (err <= t).all(), (what, "worst error / bound", float((err / t).max()) if t > 0 else err.max(), got[np.argmax(err.max(axis=1))], star[np.argmax(err.max(axis=1))])
    assert (np.abs(energy(got) - energy(star)) <= energy_bound(star, t)).all(), (what, "energy")


# ---- recorded values ----
def _hex(x):
    return None if x != x else float(x).hex()


def fixtures():
    return json.load(open(os.path.join(HERE, "golden", "energy_fixtures.json")))["cases"]


def fixture_child(c):
    """The child as the reference read it: (names, Lists over the chromosomes, overlapping)."""
    L = Lists.from_segments([(r["start"], r["finish"], [_num(x) for x in r["value"]]) for r in c["chroms"]])
    return [r["name"] for r in c["chroms"]], L, bool(c["overlaps"])


def union(L):
    """The reference's UnionWiggleIterator (unaryOps.c:60-96) per segment: a run joins the group while group.finish > start; the
    group keeps its first run's value."""
    segs = []
    for s, f, v in L.segments():
        os_, of, ov = [], [], []
        for a, b, x in zip(s, f, v):
            if os_ and of[-1] > a:
                of[-1] = max(of[-1], int(b))
            else:
                os_.append(int(a)); of.append(int(b)); ov.append(float(x))
        segs.append((os_, of, ov))
    return Lists.from_segments(segs)


def fixture_lists(c):
    """What the door sees: the union where the child overlaps; with a seek in the middle, the runs the integrator was served --
    the first 1 + pre of the list (its constructor pops once), then those of the window --, a segment per stretch of one
    chromosome (the reference's offset grows where the chromosome changes)."""
    names, L, over = fixture_child(c)
    U = union(L) if over else L
    sk = c.get("seek")
    if not sk:
        return U
    segs = U.segments()
    flat = [(g, i) for g in range(U.n_seg) for i in range(len(segs[g][0]))][:1 + sk["pre"]]
    g2 = names.index(sk["chrom"])
    flat += [(g2, i) for i in range(len(segs[g2][0])) if segs[g2][1][i] > sk["start"] and segs[g2][0][i] < sk["finish"]]
    out = []
    for k, (g, i) in enumerate(flat):
        if k == 0 or flat[k - 1][0] != g:
            out.append(([], [], []))
        for j in range(3):
            out[-1][j].append(segs[g][j][i])
    return Lists.from_segments(out)


def fixture_wavelengths(c):
    return [int(x) for x in c["wavelengths"]]


def fixture_exact(c):
    return np.array([[_num(r), _num(i)] for r, i in c["exact"]], np.float64)


def fixture_reference(c):
    """(n_wavelengths, 3): real, im, res as the compiled reference left them."""
    return np.array([[_num(x) for x in row] for row in c["reference"]], np.float64)


def seam_values():
    return json.load(open(os.path.join(HERE, "golden", "energy_seams.json")))["cases"]


# ---- the emulated passes and the host sweep ----
def emu_lib():
    """tests/emu/libwt_energy_emu.so, built (tests/emu/build.py) and loaded once."""
    from emu import build
    return build.load_unit("energy")


def _p(x):
    return C.c_void_p(x.ctypes.data) if x is not None else None


def call(fn, head, L, wavelengths, seg_base, dtype, tail=()):
    """A door with the C signature (..., n_seg, seg_off, seg_base, start, finish, value, [is_f64], n, wavelength, reim, end_base,
    ...): (rc, reim (n, 2), end_base); the outputs start as -1."""
    lam = np.ascontiguousarray(wavelengths, np.int32)
    out = np.full((max(len(lam), 1), 2), -1.0)
    end = np.full(1, -1, np.int64)
    sb = None if seg_base is None else np.ascontiguousarray(seg_base, np.int64)
    v = np.ascontiguousarray(L.v, np.float64 if dtype is None else dtype)
    f64 = [] if dtype is None else [C.c_int(1 if v.dtype == np.float64 else 0)]
    rc = fn(*head, C.c_int64(L.n_seg), _p(L.seg), _p(sb), _p(L.s), _p(L.f), _p(v), *f64, C.c_int32(len(lam)), _p(lam), _p(out), _p(end), *tail)
    return rc, out, int(end[0])


def emu_door(L, wavelengths, seg_base=None, dtype=np.float64, order=0, seed=1):
    """wen_door over the CPU launcher."""
    return call(emu_lib().energy_emu_door, [C.c_int(order), C.c_uint64(seed)], L, wavelengths, seg_base, dtype, [None])


def host_sweep(L, wavelengths, seg_base=None, dtype=np.float64):
    """wen_host (values as doubles)."""
    L2 = Lists(L.seg, L.s, L.f, np.ascontiguousarray(L.v, dtype).astype(np.float64))
    return call(emu_lib().energy_host, [], L2, wavelengths, seg_base, None)


# ---- seam cases ----
def _runs(rng, n, first=1, lengths=(1, 2, 3, 5, 10, 40), gaps=9):
    """n sorted disjoint runs from `first` on, values multiples of 1/8 (exact in float32)."""
    ln = np.asarray(lengths)[rng.integers(0, len(lengths), n)]
    gap = rng.integers(0, gaps, n)
    s = first + np.cumsum(gap + np.concatenate([[0], ln[:-1]])) if n else np.zeros(0, np.int64)
    return s.astype(np.int32), (s + ln).astype(np.int32), rng.integers(-40, 41, n) / 8.0


def seam_cases():
    """{name: (Lists, wavelengths, seg_base or None)}: every size at which the passes take another path.  All values are exact
    in float32.  The exact sums are recorded in tests/golden/energy_seams.json by the generator."""
    c = constants()
    S, B, K, BL = c["SHARE"], c["BATCH"], c["KCHUNK"], c["BLOCK"]
    rng = np.random.default_rng(20261201)
    out = {}
    two = [10, 147]
    for n in (0, 1, B - 1, B + 1, B * BL - 1, B * BL + 1, S - 1, S, S + 1, 3 * S + 1):
        out["runs_%d" % n] = (Lists.from_segments([_runs(rng, n)]), two, None)
    # segment boundaries inside a share, an empty segment between two full ones, a short last one
    out["segments"] = (Lists.from_segments([_runs(rng, S - 5), _runs(rng, 0), _runs(rng, S + 7), _runs(rng, 3)]), [7, 200], None)
    # wavelength counts around the chunk, a repeated wavelength, the small and the large ones, one equal to a run's length
    small = Lists.from_segments([_runs(rng, 300), _runs(rng, 411, first=-50)])         # (a negative start)
    pool = [1, 2, 3, 40, 7, 10, 147, 200, 1000, 2 ** 31 - 1, 10, 65537, 5, 4096, 4097, 2 ** 30 + 1, 999983, 3, 1]
    for k in (1, K - 1, K, K + 1, 2 * K + 1):
        out["wavelengths_%d" % k] = (small, (pool * 2)[:k] if k > 1 else [40], None)
    out["wavelengths_tail"] = (small, pool[K:], None)
    # positions: a base past 2^31 given explicitly, a finish at WTAMD_MAX_COORD, lengths of 1 and of 2^30
    s = np.array([-7, 5, 6, 2 ** 30 + 6, MAX_COORD - 1], np.int32)
    f = np.array([5, 6, 2 ** 30 + 6, 2 ** 30 + 7, MAX_COORD], np.int32)
    far = Lists.from_segments([(s, f, [1.5, -2.0, 0.125, 3.0, 1.0]), _runs(rng, 9)])
    out["far"] = (far, [1, 2, 3, 10, 147, 2 ** 30, 2 ** 31 - 1], None)
    out["far_base"] = (far, [2, 3, 10, 147, 2 ** 31 - 1], [3 * 10 ** 9, -(2 ** 61)])
    # NaN in the first run, in the last run of a share, and an infinity
    for name, at, x in (("nan_first", 0, np.nan), ("nan_share_end", S - 1, np.nan), ("inf", S + 3, np.inf)):
        L = Lists.from_segments([_runs(rng, S + 9)])
        L.v[at] = x
        out[name] = (L, [3, 10], None)
    for name, (L, lam, sb) in out.items():
        assert np.array_equal(L.v.astype(np.float32).astype(np.float64), L.v, equal_nan=True), name
    return out


def refusals():
    """[(name, Lists, wavelengths, seg_base)]: calls the door refuses with WTAMD_ERR_ARG before it writes anything.  The
    offending run lies in the second workgroup's share."""
    c = constants()
    S = c["SHARE"]
    rng = np.random.default_rng(20261202)

    def lists():
        return Lists.from_segments([_runs(rng, S + 10), _runs(rng, 5)])

    good = lists()
    empty, inv, unsorted, overlap = lists(), lists(), lists(), lists()
    empty.f[S + 5] = empty.s[S + 5]
    inv.f[S + 5] = inv.s[S + 5] - 1
    unsorted.s[S + 5], unsorted.f[S + 5] = unsorted.s[S + 3], unsorted.s[S + 3] + 1
    overlap.s[S + 5] = overlap.f[S + 4] - 1
    return [("no wavelength", good, [], None), ("too many wavelengths", good, [10] * (c["MAX_WAVELENGTHS"] + 1), None),
            ("wavelength 0", good, [10, 0], None), ("a negative wavelength", good, [-3], None),
            ("start == finish", empty, [10], None), ("start > finish", inv, [10], None),
            ("not sorted", unsorted, [10], None), ("overlapping", overlap, [10], None),
            ("a base beyond 2^62", good, [10], [0, 2 ** 62]), ("a base below -2^62", good, [10], [-(2 ** 62), 0])]


def check_split(door, L, lam, star, S, cuts, what):
    """Per segment: every part gets the end_base of the part before it.  Cut at `cuts` inside segments: a part that continues a
    segment keeps that segment's base.  The parts' sums added: within the bound of the exact value; the last end_base: that
    of the single call."""
    base, end_all = bases(L)
    acc, end = np.zeros((len(lam), 2)), 0
    for g in range(L.n_seg):
        rc, out, end = door(L.segment(g), lam, [end], np.float64)
        assert rc == 0, (what, g)
        acc += out
    assert end == end_all, (what, end, end_all)
    check_close(acc, star, len(L.s), S, (what, "per segment"))
    edges = [0] + sorted(cuts) + [len(L.s)]
    acc = np.zeros((len(lam), 2))
    for a, b in zip(edges[:-1], edges[1:]):
        rc, out, end = door(L.part(a, b), lam, base, np.float32)
        assert rc == 0, (what, a, b)
        acc += out
    assert end == end_all, (what, end, end_all)
    check_close(acc, star, len(L.s), S, (what, "inside a segment"))


def check_refusals(door, err):
    """Every refusal returns `err` and leaves the sentinel-filled outputs as they were.  door(L, wavelengths, seg_base, dtype)
    -> (rc, reim, end_base)."""
    for name, L, lam, sb in refusals():
        for dt in (np.float32, np.float64):
            rc, out, end = door(L, lam, sb, dt)
            assert rc == err, (name, rc)
            assert (out == -1.0).all() and end == -1, (name, out, end)
