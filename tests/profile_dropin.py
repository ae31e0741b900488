"""What tests/test_profile_model.py (the emulated drop-in library: host sweep) and tests/test_profile_gpu.py (the product)
share: a ctypes driver of wtamd_ProfileMultiplexer over NumPy arrays, read by popMultiplexer, under SelectReduction, after a
seekMultiplexer and with a MeanReduction of this library as the dataset -- against the recorded fixtures and the model."""
import ctypes as C

import numpy as np

import apply_dropin
import apply_model as AM
import exact
import profile_model as M
from apply_dropin import Multiplexer


class DropIn(apply_dropin.DropIn):
    def __init__(self, path):
        super().__init__(path)
        self.L.wtamd_ProfileMultiplexer.restype = C.c_void_p
        self.L.wtamd_ProfileMultiplexer.argtypes = [C.c_void_p, C.c_int, C.c_void_p]

    def profile(self, regions, width, dataset):
        return self.L.wtamd_ProfileMultiplexer(regions, int(width), dataset)


def _check_rows(rows, names, case, W, default, what, rec=None, stops=None):
    """Rows of a drop-in Multiplexer against the model (and, where the reference's group seek did not cut the dataset short,
    against the recording itself by the same check)."""
    exp = M.Expected(case)
    seg_of = np.repeat(np.arange(len(case.regions)), np.diff(case.rseg))
    assert [(r[0], r[1], r[2]) for r in rows] == [(names[g], int(a), int(b)) for g, a, b in zip(seg_of, case.rs, case.rf)], what
    got = np.array([r[3] for r in rows], np.float64).reshape(len(rows), W)
    exp.check(got, W, default, what)
    if rec is not None:
        for i, bins in enumerate(exp.rows(W, default)):
            s, f, _ = case.data[seg_of[i]]
            if not (f[s < case.rf[i]] > stops[i]).any():
                M.check_row(rec[i], bins, (what, i, "recorded"))
                assert all(exact.same_bits(float(x), float(y)) for x, y, b in zip(got[i], rec[i], bins) if b.exact), (what, i, "recorded bits")
    return got


def check_dropin(D, fixtures, setenv=None):
    """The checks both backends share.  setenv(name, value): given by the product's test, which then reads every recorded
    case again with WTAMD_NO_DEVICE_PROFILE=1 and expects the device's bits."""
    seen = {"select": 0, "seek": 0, "reducer": 0}
    for c in fixtures:
        case, default, W = M.fixture_case(c)
        names, stops = c["chrom_names"], AM.reference_stops(case)
        make = lambda scale=1.0: D.profile(D.region_reader(names, case), W, D.data_reader(names, case, default, scale))   # noqa: E731
        m = make()
        w = Multiplexer.from_address(m)
        assert w.count == W and all(np.isnan(w.default_values[i]) for i in range(w.count)) and w.strict == b"\x00"
        rows = D.read_mux(m)
        got = _check_rows(rows, names, case, W, default, c["name"], M.recorded_rows(c), stops)
        if setenv:
            setenv("WTAMD_NO_DEVICE_PROFILE", "1")
            host = D.read_mux(make())
            setenv("WTAMD_NO_DEVICE_PROFILE", "0")
            assert [r[:3] for r in host] == [r[:3] for r in rows], c["name"]
            assert M.same_rows(np.array([r[3] for r in host], np.float64).reshape(len(rows), W), got), c["name"]
        if int(c["name"][-3:]) % 4:
            continue
        # under SelectReduction: one bin as a WiggleIterator
        for k in sorted({0, W // 2, W - 1}):
            sel = D.read_pops(D.L.SelectReduction(make(), k))
            assert [r[:3] for r in sel] == [r[:3] for r in rows] and all(exact.same_bits(a[3], b[3][k]) for a, b in zip(sel, rows)), (c["name"], k)
            seen["select"] += 1
        # after a seekMultiplexer: both children repositioned and clipped, everything recomputed
        g = int(np.argmax(np.diff(case.rseg)))
        lo, hi = int(case.rs[case.rseg[g]]) + 1, int(case.rf[case.rseg[g]:case.rseg[g + 1]].max()) - 1
        if hi > lo:
            m = make()
            D.L.popMultiplexer(m)
            D.L.seekMultiplexer(m, names[g].encode(), lo, hi)
            _check_rows(D.read_mux(m), names, apply_dropin._clipped(case, g, lo, hi), W, default, (c["name"], "seek"))
            seen["seek"] += 1
        # a MeanReduction of this library as the dataset: the mean of x and 3x is 2x, runs and all; its default is the children's
        if not c["nan_values"] and default == default:
            kids = (C.c_void_p * 2)(D.data_reader(names, case, default), D.data_reader(names, case, default, 3.0))
            D.keep.append(kids)
            red = D.L.MeanReduction(D.L.newMultiplexer(kids, 2, b"\x00"))
            twice = AM.Case([(s, f, 2 * v) for s, f, v in case.data], case.regions, True)
            _check_rows(D.read_mux(D.profile(D.region_reader(names, case), W, red)), names, twice, W, default, (c["name"], "reducer"))
            seen["reducer"] += 1
    assert min(seen.values()) >= 15, seen
