"""What tests/test_apply_model.py (the emulated drop-in library: host sweep) and tests/test_apply_gpu.py (the product) share: a
ctypes driver of wtamd_ApplyMultiplexer over NumPy arrays, read by popMultiplexer, under SelectReduction, after a
seekMultiplexer and with a MeanReduction of this library as the dataset -- against the recorded fixtures and the model."""
import ctypes as C

import numpy as np

import apply_model as M
import cover_dropin
import exact

EXACT_STATS, VAR_STATS = ("AUC", "meanI", "maxI", "minI"), ("varI", "stddevI", "CVI")


class Multiplexer(C.Structure):
    _fields_ = [("chrom", C.c_char_p), ("start", C.c_int), ("finish", C.c_int), ("values", C.POINTER(C.c_double)),
                ("default_values", C.POINTER(C.c_double)), ("count", C.c_int), ("inplay_count", C.c_int), ("inplay", C.c_void_p),
                ("iters", C.c_void_p), ("done", C.c_char), ("strict", C.c_char), ("pop", C.c_void_p), ("seek", C.c_void_p),
                ("starts", C.c_void_p), ("finishes", C.c_void_p), ("data", C.c_void_p)]


class DropIn(cover_dropin.DropIn):
    def __init__(self, path):
        super().__init__(path)
        L = self.L
        L.wtamd_ApplyMultiplexer.restype = C.c_void_p
        L.wtamd_ApplyMultiplexer.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_char]
        L.popMultiplexer.restype = None
        L.popMultiplexer.argtypes = [C.c_void_p]
        L.seekMultiplexer.restype = None
        L.seekMultiplexer.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int]
        L.SelectReduction.restype = C.c_void_p
        L.SelectReduction.argtypes = [C.c_void_p, C.c_int]

    def data_reader(self, names, case, default, scale=1.0):
        """The dataset of a Case as wtamd_ArrayReader over the chromosomes that have runs (f32 values, the default given)."""
        has = [g for g in range(len(names)) if len(case.data[g][0])]
        arr = (C.c_char_p * max(len(has), 1))(*[names[g].encode() for g in has])
        so = np.concatenate([[0], np.cumsum([len(case.data[g][0]) for g in has])]).astype(np.int64)
        s, f = np.ascontiguousarray(case.s), np.ascontiguousarray(case.f)
        v = np.ascontiguousarray(case.v * scale, np.float32)
        self.keep.append((arr, so, s, f, v))
        return self.L.wtamd_ArrayReader(len(has), arr, so.ctypes.data, s.ctypes.data, f.ctypes.data, v.ctypes.data, float(default))

    def region_reader(self, names, case):
        has = [g for g in range(len(names)) if len(case.regions[g][0])]
        so = np.concatenate([[0], np.cumsum([len(case.regions[g][0]) for g in has])]).astype(np.int64)
        return self.reader([names[g] for g in has], so, case.rs, case.rf, np.ones(len(case.rs), np.float32), overlapping=True)       # (a BED reader: regions may overlap)

    def apply(self, regions, stats, dataset, strict):
        codes = (C.c_int * len(stats))(*[M.STATS.index(s) for s in stats])
        return self.L.wtamd_ApplyMultiplexer(regions, codes, len(stats), dataset, b"\x01" if strict else b"\x00")

    def read_mux(self, m):
        """[(chrom, start, finish, [values])] by popMultiplexer."""
        w = Multiplexer.from_address(m)
        out = []
        while w.done == b"\x00":
            out.append((w.chrom.decode(), w.start, w.finish, [w.values[i] for i in range(w.count)]))
            self.L.popMultiplexer(m)
        return out


def _check_rows(rows, names, case, default, strict, stats, what, rec=None, stops=None):
    """Rows of a drop-in Multiplexer against the model (and, where the reference's group seek did not cut the dataset short,
    the exact statistics against the recording itself)."""
    exp = case.expected(default, strict)
    seg_of = np.repeat(np.arange(len(case.regions)), np.diff(case.rseg))
    assert [(r[0], r[1], r[2]) for r in rows] == [(names[g], int(a), int(b)) for g, a, b in zip(seg_of, case.rs, case.rf)], what
    for i, (row, (m, tb, _)) in enumerate(zip(rows, exp)):
        for q, x in zip(stats, row[3]):
            if q in EXACT_STATS:
                assert exact.same_bits(x, M.finish(m, q)), (what, i, q)
                s, f, _ = case.data[seg_of[i]]
                if rec is not None and not (f[s < case.rf[i]] > stops[i]).any():
                    assert exact.same_bits(x, M.recorded(rec, q)[i]), (what, i, q, "recorded")
            else:       # T within tb of the exact value; the closing arithmetic adds a few roundings
                assert exact.rel_err(x, M.finish(m, q)) <= tb + 1e-14, (what, i, q)


def _clipped(case, g, lo, hi):
    """Chromosome g of a case as the readers deliver it after seek(lo, hi): what intersects [lo, hi), clipped."""
    s, f, v = case.data[g]
    rs, rf = case.regions[g]
    k, rk = (f > lo) & (s < hi), (rf > lo) & (rs < hi)
    n = len(case.data)
    empty_d, empty_r = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0)), (np.zeros(0, np.int32), np.zeros(0, np.int32))
    data, regs = [empty_d] * n, [empty_r] * n
    data[g] = (np.maximum(s[k], lo).astype(np.int32), np.minimum(f[k], hi).astype(np.int32), v[k])
    regs[g] = (np.maximum(rs[rk], lo).astype(np.int32), np.minimum(rf[rk], hi).astype(np.int32))
    return M.Case(data, regs, True)


def check_dropin(D, fixtures, setenv=None):
    """The checks both backends share.  setenv(name, value): given by the product's test, which then reads every recorded
    case again with WTAMD_NO_DEVICE_APPLY=1 and expects the device's bits."""
    seen = {"select": 0, "seek": 0, "reducer": 0}
    for c in fixtures:
        case, default = M.fixture_case(c)
        names, stops = c["chrom_names"], M.reference_stops(case)
        for mode, strict in (("strict", True), ("fillin", False)):
            stats = [q for q in M.STATS if q in c[mode]]
            make = lambda st=stats, scale=1.0: D.apply(D.region_reader(names, case), st, D.data_reader(names, case, default, scale), strict)   # noqa: E731
            m = make()
            w = Multiplexer.from_address(m)
            assert w.count == len(stats) and all(np.isnan(w.default_values[i]) for i in range(w.count))
            rows = D.read_mux(m)
            _check_rows(rows, names, case, default, strict, stats, (c["name"], mode), c[mode], stops)
            if setenv:
                setenv("WTAMD_NO_DEVICE_APPLY", "1")
                host = D.read_mux(make())
                setenv("WTAMD_NO_DEVICE_APPLY", "0")
                assert [r[:3] for r in host] == [r[:3] for r in rows], c["name"]
                assert M.same_rows(np.array([r[3] for r in host]).reshape(len(rows), -1), np.array([r[3] for r in rows]).reshape(len(rows), -1)), c["name"]
            if int(c["name"][-3:]) % 5:
                continue
            # under SelectReduction: one statistic as a WiggleIterator
            for k, q in enumerate(stats):
                sel = D.read_pops(D.L.SelectReduction(make(), k))
                assert [r[:3] for r in sel] == [r[:3] for r in rows] and all(exact.same_bits(a[3], b[3][k]) for a, b in zip(sel, rows)), (c["name"], q)
                seen["select"] += 1
            # after a seekMultiplexer: both children repositioned and clipped, everything recomputed
            g = int(np.argmax(np.diff(case.rseg)))
            lo, hi = int(case.rs[case.rseg[g]]) + 1, int(case.rf[case.rseg[g]:case.rseg[g + 1]].max()) - 1
            if hi > lo:
                m = make()
                D.L.popMultiplexer(m)
                D.L.seekMultiplexer(m, names[g].encode(), lo, hi)
                _check_rows(D.read_mux(m), names, _clipped(case, g, lo, hi), default, strict, stats, (c["name"], mode, "seek"))
                seen["seek"] += 1
            # a MeanReduction of this library as the dataset: the mean of x and 3x is 2x, runs and all; its default is the children's
            if not c["nan_values"] and default == default:
                kids = (C.c_void_p * 2)(D.data_reader(names, case, default), D.data_reader(names, case, default, 3.0))
                D.keep.append(kids)
                red = D.L.MeanReduction(D.L.newMultiplexer(kids, 2, b"\x00"))
                twice = M.Case([(s, f, 2 * v) for s, f, v in case.data], case.regions, True)
                _check_rows(D.read_mux(D.apply(D.region_reader(names, case), stats, red, strict)), names, twice, default, strict, stats,
                            (c["name"], mode, "reducer"))
                seen["reducer"] += 1
    assert min(seen.values()) >= 20, seen
