"""NumPy model of the reference's region operators (src/unaryOps.c:437-639: OverlapWiggleIterator, NoverlapWiggleIterator,
TrimWiggleIterator, NearestWiggleIterator) over one segment (= one chromosome) of a source and a mask, both sorted by start,
and the helpers the region tests share.

With G = union(M) (cover_model.union: touching intervals stay apart), lo(i) = the first group with G.finish > S.start[i] and
hi(i) = the first group with G.start >= S.finish[i]:
  overlaps   run i iff hi > lo                       noverlaps   run i iff hi <= lo
  trim       for g in [lo, hi): [max(S.start, G.start[g]), min(S.finish, G.finish[g])) with the value of run i
  nearest    k = #(M.start <= S.start[i]) over the raw mask; the smaller of S.start - M.finish[k-1] + 1 (k > 0) and
             M.start[k] - S.finish + 1 (k < m) in int32 arithmetic, 0 where negative, NaN without a candidate.
trim_protocol is the reference's own pop protocol for a trim, which differs from the rule when the SOURCE overlaps itself."""
import ctypes as C
import os
import re

import numpy as np

import cover_model as CM

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "wiggletools_amd", "csrc", "wt_region.h")

OPS = {"overlaps": 0, "noverlaps": 1, "trim": 2, "nearest": 3}
same_bits = CM.same_bits


def _empty():
    return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64)


def region(op, start, finish, value, m_start, m_finish):
    """One segment; value of any float dtype, returned as float64 (widened exactly)."""
    op = OPS[op] if isinstance(op, str) else int(op)
    s, f = np.asarray(start, np.int64), np.asarray(finish, np.int64)
    v = np.asarray(value).astype(np.float64)
    ms, mf = np.asarray(m_start, np.int64), np.asarray(m_finish, np.int64)
    if len(s) == 0:
        return _empty()
    if op == 3:
        k = np.searchsorted(ms, s, side="right")
        big = np.int64(1) << 40
        prev = np.where(k > 0, (s - mf[np.maximum(k - 1, 0)] + 1) if len(ms) else big, big)
        nxt = np.where(k < len(ms), (ms[np.minimum(k, len(ms) - 1)] - f + 1) if len(ms) else big, big)
        best = np.minimum(prev, nxt)
        out = np.where(best == big, np.nan, np.maximum(best, 0).astype(np.float64))
        return s.astype(np.int32), f.astype(np.int32), out
    gs, gf, _ = CM.union(ms, mf, np.zeros(len(ms)))
    gs, gf = gs.astype(np.int64), gf.astype(np.int64)
    lo = np.searchsorted(gf, s, side="right")          # the first group with finish > start
    hi = np.searchsorted(gs, f, side="left")           # the first group with start >= finish
    if op in (0, 1):
        keep = (hi > lo) if op == 0 else (hi <= lo)
        return s[keep].astype(np.int32), f[keep].astype(np.int32), v[keep]
    cnt = np.maximum(hi - lo, 0)
    src = np.repeat(np.arange(len(s)), cnt)
    grp = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(lo, cnt)
    return np.maximum(s[src], gs[grp]).astype(np.int32), np.minimum(f[src], gf[grp]).astype(np.int32), v[src]


def trim_protocol(start, finish, value, m_start, m_finish):
    """TrimWiggleIterator's pop protocol (unaryOps.c:485-516) over one chromosome: the mask goes through the union first
    (:521); after an output the side that ends first is popped."""
    gs, gf, _ = CM.union(np.asarray(m_start, np.int64), np.asarray(m_finish, np.int64), np.zeros(len(m_start)))
    s, f, v = np.asarray(start), np.asarray(finish), np.asarray(value).astype(np.float64)
    i = g = 0
    os_, of, ov = [], [], []
    while i < len(s) and g < len(gs):
        if gf[g] <= s[i]:
            g += 1
        elif f[i] <= gs[g]:
            i += 1
        else:
            os_.append(max(s[i], gs[g])); of.append(min(f[i], gf[g])); ov.append(v[i])
            if f[i] <= gf[g]:
                i += 1
            else:
                g += 1
    return np.array(os_, np.int32), np.array(of, np.int32), np.array(ov, np.float64)


def segmented(op, seg_off, start, finish, value, m_seg_off, m_start, m_finish, fn=region):
    """The model over every segment pair; returns (o_seg_off, start, finish, value)."""
    outs, off = [], [0]
    for g in range(len(seg_off) - 1):
        a, b, ma, mb = int(seg_off[g]), int(seg_off[g + 1]), int(m_seg_off[g]), int(m_seg_off[g + 1])
        r = fn(op, start[a:b], finish[a:b], value[a:b], m_start[ma:mb], m_finish[ma:mb]) if fn is region else \
            fn(start[a:b], finish[a:b], value[a:b], m_start[ma:mb], m_finish[ma:mb])
        outs.append(r)
        off.append(off[-1] + len(r[0]))
    cat = lambda k, dt: np.concatenate([o[k] for o in outs]).astype(dt) if outs else np.zeros(0, dt)   # noqa: E731
    return np.array(off, np.int64), cat(0, np.int32), cat(1, np.int32), cat(2, np.float64)


def overlaps_itself(seg_off, start, finish):
    """Some run starts before the run in front of it, in the same segment, has ended."""
    return any(bool((start[a + 1:b] < finish[a:b - 1]).any()) for a, b in zip(seg_off[:-1], seg_off[1:]) if b - a > 1)


def constants():
    """(T, W): source runs per tile and the LDS mask window of csrc/wt_region.h."""
    txt = open(HEADER).read()
    block = int(re.search(r"#define WCV_BLOCK (\d+)", open(os.path.join(os.path.dirname(HEADER), "wt_cover.h")).read()).group(1))
    per = int(re.search(r"#define WRG_PER_LANE (\d+)", txt).group(1))
    return block * per, int(re.search(r"#define WRG_WINDOW (\d+)", txt).group(1))


def disjoint_segment(rng, n, span, touching=0.3):
    """n sorted runs that do not overlap inside [1, 1 + span]; some touch."""
    n = int(n)
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    cuts = np.sort(rng.choice(np.arange(1, span + 2), size=min(2 * n, span + 1), replace=False))
    cuts = cuts[:2 * (len(cuts) // 2)]
    s, f = cuts[0::2].copy(), cuts[1::2].copy()
    t = np.nonzero(rng.random(len(s)) < touching)[0]
    t = t[t > 0]
    s[t] = f[t - 1]
    return s.astype(np.int32), f.astype(np.int32)


def flat(segs):
    seg_off = np.concatenate([[0], np.cumsum([len(x[0]) for x in segs])]).astype(np.int64)
    cat = lambda k: np.concatenate([x[k] for x in segs]).astype(np.int32) if segs else np.zeros(0, np.int32)   # noqa: E731
    return seg_off, cat(0), cat(1)


def values(n, dt, seed=1):
    """Values whose bits must arrive unchanged: NaN (with a payload in f64), -0.0, denormal, the rest random."""
    v = np.random.default_rng(seed).standard_normal(n).astype(dt)
    special = [np.nan, -0.0, np.finfo(dt).tiny / 4]
    if dt == np.float64:
        special.append(np.array([0x7ff8000000000123], np.uint64).view(np.float64)[0])
    for k, x in enumerate(special):
        v[k::max(n // 3, len(special))] = x
    return v


def seam_cases():
    """{name: (source segments, mask segments)} at the sizes where the passes change tile, lane or search path (also run
    on the device).  T source runs make a tile; a tile stages up to W mask groups in LDS."""
    T, W = constants()
    rng = np.random.default_rng(6)
    out = {}
    empty = (np.zeros(0, np.int32), np.zeros(0, np.int32))
    for n in (T - 1, T, T + 1, 3 * T + 5):
        out["n%d" % n] = ([disjoint_segment(rng, n, 12 * n)], [CM.random_segment(rng, n // 3, 12 * n, 40)])
        out["n%d_overlapping" % n] = ([CM.random_segment(rng, n, 12 * n, 60)], [CM.random_segment(rng, n // 2, 12 * n, 30)])
    # one tile of T - 3 runs over a mask of exactly W and of W + 1 disjoint groups, every group met
    for w in (W, W + 1):
        ms = (10 + 4 * np.arange(w)).astype(np.int32)
        mask = (ms, (ms + 2).astype(np.int32))
        edges = np.linspace(5, 10 + 4 * w + 5, T - 2).astype(np.int64)
        out["window%d" % w] = ([(edges[:-1].astype(np.int32), edges[1:].astype(np.int32))], [mask])
    # the last run of the first tile meets 2T + 3 groups; the tile after it goes on
    ns = T
    s = (1 + 3 * np.arange(ns - 1)).astype(np.int64)
    f = s + 2
    g0 = int(f[-1]) + 5
    gs = g0 + 3 * np.arange(2 * T + 3)
    big = (g0 - 2, int(gs[-1]) + 2)
    tail = big[1] + 4 * np.arange(1, 40)
    src = (np.concatenate([s, [big[0]], tail]).astype(np.int32), np.concatenate([f, [big[1]], tail + 3]).astype(np.int32))
    msk = (np.concatenate([[2, 9], gs, tail[::3] + 1]).astype(np.int32), np.concatenate([[4, 30], gs + 2, tail[::3] + 9]).astype(np.int32))
    out["wide_trim"] = ([src], [msk])
    # several segments inside one tile: an empty source, an empty mask, both empty, and ordinary ones
    a, b, c = (disjoint_segment(rng, k, 900) for k in (40, 7, 90))
    out["segments"] = ([a, empty, b, empty, c, disjoint_segment(rng, 3, 50)],
                       [CM.random_segment(rng, 20, 900, 30), CM.random_segment(rng, 9, 900, 30), empty, empty,
                        CM.random_segment(rng, 50, 900, 12), CM.random_segment(rng, 1, 50, 5)])
    out["segments_many"] = ([disjoint_segment(rng, int(rng.integers(0, 200)), 3000) if k % 5 else empty for k in range(40)],
                            [CM.random_segment(rng, int(rng.integers(0, 90)), 3000, 50) if k % 3 else empty for k in range(40)])
    # strictness: a run that starts where a group ends, and one that ends where a group starts, meet neither
    out["strict"] = ([(np.array([5, 20, 30, 40], np.int32), np.array([10, 30, 40, 50], np.int32))],
                     [(np.array([1, 10, 40, 50], np.int32), np.array([5, 20, 41, 60], np.int32))])
    # nearest: M.start == S.start, k = 0, k = m, an overlap clamped to 0, an enclosing earlier mask that is not seen
    out["nearest"] = ([(np.array([3, 10, 25, 100, 200], np.int32), np.array([5, 12, 40, 120, 210], np.int32))],
                      [(np.array([10, 20, 22, 90, 150], np.int32), np.array([11, 500, 23, 110, 160], np.int32))])
    out["nearest_no_mask"] = ([(np.array([3, 10], np.int32), np.array([5, 12], np.int32))], [empty])
    return out


# ---- the passes of csrc/wt_region.h on the CPU (tests/region_emu.cpp) ----
def emu_lib():
    """tests/emu/libwt_region_emu.so, built (tests/emu/build.py) and loaded once."""
    from emu import build
    return build.load_unit("region")


def default_capacity(op, n, m):
    op = OPS[op] if isinstance(op, str) else int(op)
    return n + m if op == 2 else n


def emu_region(op, seg_off, start, finish, value, m_seg_off, m_start, m_finish, order=0, seed=0, capacity=None):
    """Returns (rc, n_out, o_seg_off, start, finish, value, untouched); the output arrays start out filled with -1, and
    `untouched` says that a refused call left them so."""
    L = emu_lib()
    op = OPS[op] if isinstance(op, str) else int(op)
    seg_off, m_seg_off = np.ascontiguousarray(seg_off, np.int64), np.ascontiguousarray(m_seg_off, np.int64)
    start, finish = np.ascontiguousarray(start, np.int32), np.ascontiguousarray(finish, np.int32)
    m_start, m_finish = np.ascontiguousarray(m_start, np.int32), np.ascontiguousarray(m_finish, np.int32)
    value = np.ascontiguousarray(value)
    assert value.dtype in (np.float32, np.float64)
    cap = default_capacity(op, len(start), len(m_start)) if capacity is None else capacity
    os_, of, ov = np.full(max(cap, 1), -1, np.int32), np.full(max(cap, 1), -1, np.int32), np.full(max(cap, 1), -1.0, np.float64)
    oseg = np.full(len(seg_off), -1, np.int64)
    n_out = C.c_int64(-1)
    p = lambda a: C.c_void_p(a.ctypes.data)     # noqa: E731
    rc = L.region_emu(C.c_int(order), C.c_uint64(seed), C.c_int(op), C.c_int64(len(seg_off) - 1), p(seg_off), p(start), p(finish), p(value),
                      C.c_int(int(value.dtype == np.float64)), p(m_seg_off), p(m_start), p(m_finish), C.c_int64(cap), p(os_), p(of), p(ov),
                      p(oseg), C.byref(n_out))
    if rc != 0:
        untouched = bool((os_ == -1).all() and (of == -1).all() and (ov == -1.0).all())
        return rc, n_out.value, oseg, os_[:0], of[:0], ov[:0], untouched
    m = n_out.value
    return rc, m, oseg, os_[:m], of[:m], ov[:m], True
