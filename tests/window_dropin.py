"""What tests/test_window_dropin_host.py (the emulated drop-in library: host sweeps) and tests/test_window_gpu.py (the product)
share: a ctypes driver of wtamd_BinIterator and wtamd_SmoothIterator over NumPy arrays, read by pop() and in blocks, after a
seek, under a SumReduction of this library and over an overlapping child -- against the recorded fixtures and the model."""
import ctypes as C
import os

import numpy as np

import cover_dropin
import window_model as M


class DropIn(cover_dropin.DropIn):
    def __init__(self, path):
        super().__init__(path)
        for name in ("wtamd_BinIterator", "wtamd_SmoothIterator"):
            getattr(self.L, name).restype = C.c_void_p
            getattr(self.L, name).argtypes = [C.c_void_p, C.c_int]
        self.L.SumReduction.restype = C.c_void_p
        self.L.SumReduction.argtypes = [C.c_void_p]

    def child(self, names, case, default, overlapping=False):
        """A Case as wtamd_ArrayReader (or the overlapping reader) over the chromosomes that have runs: f32 values."""
        has = [g for g in range(len(case.chroms)) if len(case.chroms[g][0])]
        arr = (C.c_char_p * max(len(has), 1))(*[names[g].encode() for g in has])
        so = np.concatenate([[0], np.cumsum([len(case.chroms[g][0]) for g in has])]).astype(np.int64)
        s, f, v = np.ascontiguousarray(case.s), np.ascontiguousarray(case.f), np.ascontiguousarray(case.v, np.float32)
        self.keep.append((arr, so, s, f, v))
        fn = self.L.wtamd_OverlappingArrayReader if overlapping else self.L.wtamd_ArrayReader
        return fn(len(has), arr, so.ctypes.data, s.ctypes.data, f.ctypes.data, v.ctypes.data, float(default))

    def window(self, op, child, width):
        return (self.L.wtamd_BinIterator if op == "bin" else self.L.wtamd_SmoothIterator)(child, int(width))


def _same(got, exp, what):
    assert [r[:3] for r in got] == [r[:3] for r in exp], what
    assert M.same_bits([r[3] for r in got], [r[3] for r in exp]), what


def _model_rows(op, case, names, w, default):
    rows = M.bin(case.chroms, w, default) if op == "bin" else M.smooth(case.chroms, w)
    return [(names[c], s, f, t.float()) for c, s, f, t in rows]


def _case_of(rows, names):
    """What a child delivered by pop() as a Case over `names`."""
    return M.Case([([r[1] for r in rows if r[0] == n], [r[2] for r in rows if r[0] == n], [r[3] for r in rows if r[0] == n]) for n in names])


def _union(case):
    """UnionWiggleIterator per chromosome: a run joins the group while group.finish > start."""
    out = []
    for s, f, v in case.chroms:
        gs, gf, gv = [], [], []
        for a, b, x in zip(s.tolist(), f.tolist(), v.tolist()):
            if gs and gf[-1] > a:
                gf[-1] = max(gf[-1], b)
            else:
                gs.append(a); gf.append(b); gv.append(x)
        out.append((gs, gf, gv))
    return M.Case(out)


def check_dropin(D, fixtures, setenv=None):
    """The checks both backends share.  setenv(name, value): given by the product's test, which then reads every recorded case
    again with WTAMD_NO_DEVICE_WINDOW=1 and expects the device's bits."""
    seen = {"seek": 0, "reducer": 0, "overlap": 0, "blocks": 0}
    for c in fixtures:
        case, default, w = M.fixture_case(c)
        names = c["chrom_names"]
        k = int(c["name"][-3:])
        for op in ("bin", "smooth"):
            make = lambda: D.window(op, D.child(names, case, default), w)      # noqa: E731
            wi = make()
            fields = D.fields(wi)
            assert fields.overlaps == b"\x00" and M.same_bits([fields.default_value], [M._num(c[op]["default"])]), (c["name"], op)
            rows = D.read_pops(wi)
            _same(rows, [(names[r[0]],) + r[1:] for r in M.recorded(c[op])], (c["name"], op))
            if setenv:
                setenv("WTAMD_NO_DEVICE_WINDOW", "1")
                host = D.read_pops(make())
                setenv("WTAMD_NO_DEVICE_WINDOW", "0")
                _same(host, rows, (c["name"], op, "host"))
            if k % 4:
                continue
            if op == "smooth":                  # served in clip slices of 37 positions: the same run list
                os.environ["WTAMD_WINDOW_SLICE"] = "37"
                try:
                    _same(D.read_pops(make()), rows, (c["name"], op, "slices"))
                finally:
                    del os.environ["WTAMD_WINDOW_SLICE"]
            _same(D.read_blocks(make(), pops_between=2), rows, (c["name"], op, "blocks"))
            seen["blocks"] += 1
            # after a seek: the child repositioned, everything recomputed over what it then delivers
            g = int(np.argmax(np.diff(case.seg)))
            s, f, _ = case.chroms[g]
            lo, hi = int(s[0]) + 1, int(f[-1]) - 1
            if hi > lo:
                wi = make()
                D.L.pop(wi)
                D.seek(wi, names[g], lo, hi)
                kid = D.child(names, case, default)
                D.seek(kid, names[g], lo, hi)
                _same(D.read_pops(wi), _model_rows(op, _case_of(D.read_pops(kid), names), names, w, default), (c["name"], op, "seek"))
                seen["seek"] += 1
            if np.isnan(case.v).any():
                continue
            # under a SumReduction of this library: the Multiplexer takes the doubles the iterators pop
            kids = (C.c_void_p * 2)(make(), make())
            D.keep.append(kids)
            red = D.read_pops(D.L.SumReduction(D.L.newMultiplexer(kids, 2, b"\x00")))
            ok = [r for r in rows if r[3] == r[3]]
            if len(ok) == len(rows):
                assert [r[:3] for r in red] == [r[:3] for r in rows], (c["name"], op, "reducer")
                assert all(x[3] == 2.0 * r[3] for x, r in zip(red, rows)), (c["name"], op, "reducer")
                seen["reducer"] += 1
            # over an overlapping child: the union comes first
            over = M.Case([(np.repeat(s, 2), np.stack([f, f + 1 + np.arange(len(f)) % 3]).T.ravel(), np.stack([v, v + 1]).T.ravel()) for s, f, v in case.chroms])
            got = D.read_pops(D.window(op, D.child(names, over, default, overlapping=True), w))
            _same(got, _model_rows(op, _union(over), names, w, default), (c["name"], op, "overlapping"))
            seen["overlap"] += 1
    assert min(seen.values()) >= 6, seen
    # a chromosome that starts below 1: the reference's own loops on the host (C's division towards zero, the prefill)
    odd = M.Case([([-4, 3, 9], [2, 7, 12], [1.5, -2.0, 4.0])])
    for op in ("bin", "smooth"):
        for w in (2, 5):
            _same(D.read_pops(D.window(op, D.child(["chr1"], odd, 1.5), w)), _model_rows(op, odd, ["chr1"], w, 1.5), (op, w, "start < 1"))
