"""NumPy model of the reference's CoverageWiggleIterator (src/unaryOps.c:303-375) and UnionWiggleIterator (:60-92) over one
segment (= one chromosome of one track) of intervals sorted by start, and the helpers the coverage tests share.

Coverage: B = the sorted distinct starts and finishes; run [B[k], B[k+1]) with value #(start <= B[k]) - #(finish <= B[k])
wherever that is > 0 -- not merged where the depth does not change, input values ignored.  The reference additionally emits
one run with start == finish per non-empty stream (it reads the exhausted child's stale start, :333-334): strip_zero_length
removes it from recorded reference output and says how many it removed.

Union: an interval joins the current group while group.finish > start (strict); the group has the first member's start and
value and the largest finish."""
import ctypes as C

import numpy as np


def coverage(start, finish):
    start = np.asarray(start, np.int64)
    finish = np.asarray(finish, np.int64)
    if len(start) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64)
    B = np.unique(np.concatenate([start, finish]))
    ss, fs = np.sort(start), np.sort(finish)
    depth = np.searchsorted(ss, B, side="right") - np.searchsorted(fs, B, side="right")
    keep = np.nonzero(depth[:-1] > 0)[0]
    return B[keep].astype(np.int32), B[keep + 1].astype(np.int32), depth[keep].astype(np.float64)


def union(start, finish, value):
    """value: any float dtype; returned as float64 (widened exactly)."""
    start = np.asarray(start, np.int64)
    finish = np.asarray(finish, np.int64)
    value = np.asarray(value)
    n = len(start)
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64)
    pm = np.maximum.accumulate(finish)
    head = np.ones(n, bool)
    head[1:] = start[1:] >= pm[:-1]
    h = np.nonzero(head)[0]
    last = np.concatenate([h[1:], [n]]) - 1
    return start[h].astype(np.int32), pm[last].astype(np.int32), value[h].astype(np.float64)


def segmented(fn, seg_off, *arrays):
    """fn over every segment; returns (o_seg_off, start, finish, value)."""
    outs, off = [], [0]
    for g in range(len(seg_off) - 1):
        lo, hi = int(seg_off[g]), int(seg_off[g + 1])
        r = fn(*[a[lo:hi] for a in arrays])
        outs.append(r)
        off.append(off[-1] + len(r[0]))
    cat = lambda k, dt: np.concatenate([o[k] for o in outs]).astype(dt) if outs else np.zeros(0, dt)   # noqa: E731
    return np.array(off, np.int64), cat(0, np.int32), cat(1, np.int32), cat(2, np.float64)


def strip_zero_length(chrom, start, finish, value):
    """Recorded reference coverage without its runs of start == finish; also returns how many there were."""
    start, finish = np.asarray(start), np.asarray(finish)
    keep = start != finish
    return np.asarray(chrom)[keep], start[keep], finish[keep], np.asarray(value)[keep], int((~keep).sum())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def random_segment(rng, n, span, max_len):
    """n intervals sorted by start inside [1, 1 + span], with duplicates, nesting and touching intervals."""
    n = int(n)
    s = np.sort(rng.integers(1, span + 1, n))
    ln = rng.integers(1, max_len + 1, n)
    f = np.minimum(s + ln, span + 1)
    if n > 3:
        k = rng.integers(1, n, max(1, n // 8))
        s[k] = s[k - 1]                                 # shared starts (some of them exact duplicates)
        f[k] = np.where(rng.random(len(k)) < 0.5, f[k - 1], np.maximum(f[k], s[k] + 1))
        t = rng.integers(1, n, max(1, n // 8))
        s[t] = np.minimum(f[t - 1], span)               # touching: a start that is another interval's finish
        f[t] = np.maximum(f[t], s[t] + 1)
        o = np.argsort(s, kind="stable")
        s, f = s[o], f[o]
    f = np.maximum(f, s + 1)
    return s.astype(np.int32), f.astype(np.int32)


def seam_cases():
    """Shapes at which the passes change workgroup, bitmap word or rank block (also run on the device)."""
    rng = np.random.default_rng(5)
    out = {}
    for n in (1, 255, 256, 257):
        out["n%d" % n] = [random_segment(rng, n, 3000, 40)]
    for span in (63, 64, 65, 131071, 131072, 131073):
        # the bitmap starts at position 1, so position 1 + span is its bit `span`: a breakpoint exactly there, with the depth
        # back at 0 (`a`: nothing starts there, the next interval follows a gap) or not (`b`: two intervals start there)
        rs, rf = random_segment(rng, 300, span, 9)                    # (finishes <= 1 + span)
        for tag, extra in (("a", []), ("b", [(span + 1, span + 3), (span + 1, span + 2)])):
            iv = [(1, span + 1), (1, 7), (5, span + 1), (span - 1, span + 1), (span + 4, span + 6)] + extra
            s = np.concatenate([[x[0] for x in iv], rs])
            f = np.concatenate([[x[1] for x in iv], rf])
            o = np.argsort(s, kind="stable")
            out["span%d%s" % (span, tag)] = [(s[o].astype(np.int32), f[o].astype(np.int32))]
    # one interval over everything above many short ones: a carry through many blocks, empty blocks between
    s = np.concatenate([[1], np.sort(rng.integers(2, 400000, 3000))])
    f = np.concatenate([[400100], s[1:] + rng.integers(1, 4, 3000)])
    out["carry"] = [(s.astype(np.int32), f.astype(np.int32))]
    out["identical"] = [(np.full(700, 17, np.int32), np.full(700, 4000, np.int32))]
    t = np.arange(1, 5000, 7)
    out["touching"] = [(t[:-1].astype(np.int32), t[1:].astype(np.int32))]
    empty = (np.zeros(0, np.int32), np.zeros(0, np.int32))
    out["segments"] = [empty, random_segment(rng, 40, 500, 30), empty, empty, random_segment(rng, 600, 70000, 900), empty]
    out["segments50"] = [random_segment(rng, int(rng.integers(0, 30)), 2000, 50) if k % 7 else empty for k in range(50)]
    return out


def flat(segs):
    seg_off = np.concatenate([[0], np.cumsum([len(x[0]) for x in segs])]).astype(np.int64)
    return seg_off, np.concatenate([x[0] for x in segs]).astype(np.int32), np.concatenate([x[1] for x in segs]).astype(np.int32)


# ---- the passes of csrc/wt_cover.h on the CPU (tests/cover_emu.cpp) ----
def emu_lib():
    """tests/emu/libwt_cover_emu.so, built (tests/emu/build.py) and loaded once."""
    from emu import build
    return build.load_unit("cover")


def _out(cap):
    return np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.float64)


def emu_coverage(seg_off, start, finish, order=0, seed=0, capacity=None, budget=256 << 20):
    """Returns (rc, n_out, o_seg_off, start, finish, value)."""
    L = emu_lib()
    seg_off = np.ascontiguousarray(seg_off, np.int64)
    start, finish = np.ascontiguousarray(start, np.int32), np.ascontiguousarray(finish, np.int32)
    cap = max(2 * len(start), 1) if capacity is None else capacity
    os_, of, ov = _out(cap)
    oseg = np.zeros(len(seg_off), np.int64)
    n_out, launches = C.c_int64(), C.c_int64()
    rc = L.cover_emu_coverage(C.c_int(order), C.c_uint64(seed), C.c_int64(len(seg_off) - 1), C.c_void_p(seg_off.ctypes.data),
                              C.c_void_p(start.ctypes.data), C.c_void_p(finish.ctypes.data), C.c_int64(cap), C.c_void_p(os_.ctypes.data),
                              C.c_void_p(of.ctypes.data), C.c_void_p(ov.ctypes.data), C.c_void_p(oseg.ctypes.data), C.byref(n_out),
                              C.c_int64(budget), C.byref(launches))
    m = min(n_out.value, cap)
    return rc, n_out.value, oseg, os_[:m], of[:m], ov[:m], launches.value


def emu_union(seg_off, start, finish, value, order=0, seed=0, capacity=None):
    L = emu_lib()
    seg_off = np.ascontiguousarray(seg_off, np.int64)
    start, finish = np.ascontiguousarray(start, np.int32), np.ascontiguousarray(finish, np.int32)
    value = np.ascontiguousarray(value)
    assert value.dtype in (np.float32, np.float64)
    cap = max(len(start), 1) if capacity is None else capacity
    os_, of, ov = _out(cap)
    oseg = np.zeros(len(seg_off), np.int64)
    n_out = C.c_int64()
    rc = L.cover_emu_union(C.c_int(order), C.c_uint64(seed), C.c_int64(len(seg_off) - 1), C.c_void_p(seg_off.ctypes.data),
                           C.c_void_p(start.ctypes.data), C.c_void_p(finish.ctypes.data), C.c_void_p(value.ctypes.data),
                           C.c_int(int(value.dtype == np.float64)), C.c_int64(cap), C.c_void_p(os_.ctypes.data), C.c_void_p(of.ctypes.data),
                           C.c_void_p(ov.ctypes.data), C.c_void_p(oseg.ctypes.data), C.byref(n_out))
    m = min(n_out.value, cap)
    return rc, n_out.value, oseg, os_[:m], of[:m], ov[:m]
