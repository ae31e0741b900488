"""The genome-wide statistics above a reducer that need more than a sum: wtamd_VarianceIntegrator,
wtamd_StandardDeviationIntegrator, wtamd_CoefficientOfVariationIntegrator, wtamd_MaxIntegrator, wtamd_MinIntegrator and
wtamd_SpanIntegrator (reference varI / stddevI / CVI / maxI / minI, src/statistics.c:129-326, commandParser.c:653-704) --
against the COMPILED REFERENCE's integrators over the reference's reducers, both driven by tests/integ_driver.c.

Handed this library's own reducer they run ON THE DEVICE batch by batch (wtamd_pipe_set_integrate mode 2: six doubles per
batch come home); with WTAMD_NO_FUSED_INTEGRATORS=1, or on a pipeline without that mode (the emulated one), they are the
reference's per-run pass-through on the host and equal it bit for bit.

One departure: the reference's varI / stddevI / CVI never end over a source with a NaN run (VarianceCorePop returns without
popping, statistics.c:238-239), so the reference is asked for these three only where the reducer's output has no NaN; ours
skip NaN runs and are checked against a restatement of the reference's update over the non-NaN runs.

"emu": host logic over the emulated pipeline (CPU); "amd" (-m gpu): the product (HIP kernels)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import random_case
from test_integrator_doors import _close

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

REDUCERS = {"mean": "MeanReduction", "sum": "SumReduction", "max": "MaxReduction", "median": "MedianReduction",
            "var": "VarianceReduction"}
EXACT = ("mean", "sum", "max", "median")        # reducers whose values the project holds bit-exact (test_dropin.EXACT)
KINDS = {"var": "VarianceIntegrator", "stddev": "StandardDeviationIntegrator", "cv": "CoefficientOfVariationIntegrator",
         "max": "MaxIntegrator", "min": "MinIntegrator", "span": "SpanIntegrator"}
VAR_FAMILY = ("var", "stddev", "cv")


class _Tracks(C.Structure):
    _fields_ = [("n_chrom", C.c_int32), ("n_tracks", C.c_int32), ("seg_off", C.c_void_p), ("start", C.c_void_p),
                ("finish", C.c_void_p), ("value", C.c_void_p), ("defaults", C.c_void_p)]


def _pack(d):
    keep = [np.ascontiguousarray(d["seg_off"], np.int64), np.ascontiguousarray(d["start"], np.int32),
            np.ascontiguousarray(d["finish"], np.int32), np.ascontiguousarray(d["value"], np.float64),
            np.ascontiguousarray(d["defaults"], np.float64)]
    return _Tracks(int(d["n_chrom"]), int(d["n_tracks"]), *[a.ctypes.data for a in keep]), keep


_driver_so = None


def _driver_lib(tmp):
    """tests/integ_driver.c compiled with the host gcc (as test_capi_symbols.py and the oracle do); every Driver gets a
    handle of its own from it."""
    global _driver_so
    if _driver_so is None:
        so = os.path.join(str(tmp), "libinteg_driver.so")
        subprocess.check_call(["gcc", "-O1", "-std=c99", "-D_GNU_SOURCE", "-fPIC", "-shared", "-Wall", "-I", os.path.join(ROOT, "include"),
                               os.path.join(HERE, "integ_driver.c"), "-o", so, "-ldl"])
        L = C.CDLL(so)
        L.idrv_open.restype = C.c_void_p
        L.idrv_open.argtypes = [C.c_char_p]
        L.idrv_run.argtypes = [C.c_void_p, C.POINTER(_Tracks), C.c_char_p, C.c_int, C.c_char_p, C.POINTER(C.c_double), C.c_void_p]
        L.idrv_run_seek.argtypes = [C.c_void_p, C.POINTER(_Tracks), C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_void_p,
                                    C.c_void_p]
        _driver_so = L
    return _driver_so


class Driver:
    def __init__(self, L, lib_path, prefix):
        self.L, self.prefix = L, prefix
        self.h = L.idrv_open(lib_path.encode())
        assert self.h, "integ_driver could not open %s" % lib_path

    def run(self, d, kind, op="mean", flags=0):
        """(result, pops, d2h bytes, runs)"""
        s, keep = _pack(d)
        out, info = C.c_double(), np.zeros(3, np.int64)
        rc = self.L.idrv_run(self.h, C.byref(s), REDUCERS[op].encode(), flags & 1, (self.prefix + KINDS[kind]).encode(), C.byref(out),
                             info.ctypes.data)
        assert rc == 0, "idrv_run(%s, %s) returned %d (-2: symbol missing, -4: not done at the pop cap)" % (kind, op, rc)
        return out.value, int(info[0]), int(info[1]), int(info[2])

    def run_seek(self, d, kind, regions, op="mean", flags=0, pre_pops=0):
        s, keep = _pack(d)
        reg = np.ascontiguousarray(np.array(regions, np.int32).reshape(-1, 3))
        out = np.zeros(1 + len(reg), np.float64)
        rc = self.L.idrv_run_seek(self.h, C.byref(s), REDUCERS[op].encode(), flags & 1, (self.prefix + KINDS[kind]).encode(), pre_pops,
                                  len(reg), reg.ctypes.data, out.ctypes.data)
        assert rc == 0, "idrv_run_seek(%s, %s) returned %d" % (kind, op, rc)
        return out


_drivers = {}


def _get(backend, oracle, tmp):
    if backend not in _drivers:
        L = _driver_lib(tmp)
        if backend == "ref":
            _drivers[backend] = Driver(L, os.path.join(ROOT, "oracle", "_ref", "libwiggletools_ref.so"), "")
        elif backend == "amd":
            import torch
            assert torch.cuda.is_available()
            from wiggletools_amd import _lib
            _drivers[backend] = Driver(L, _lib.LIB_PATH, "wtamd_")
        else:
            from emu import build as emu_build
            _drivers[backend] = Driver(L, emu_build.build_dropin(), "wtamd_")
    return _drivers[backend]


@pytest.fixture(params=["emu", pytest.param("amd", marks=pytest.mark.gpu)])
def H(request, oracle, tmp_path_factory):
    D = _get(request.param, oracle, tmp_path_factory.getbasetemp())
    D.backend = request.param
    return D


@pytest.fixture
def R(oracle, tmp_path_factory):
    if not oracle.have_ref():
        pytest.skip("compiled reference not available")
    return _get("ref", oracle, tmp_path_factory.getbasetemp())


def _same(a, b):
    """bit for bit: -0.0 is not 0.0; the sign of a NaN is not compared"""
    if np.isnan(a) or np.isnan(b):
        return bool(np.isnan(a) and np.isnan(b))
    return a == b and np.signbit(a) == np.signbit(b)


def _rel(a, b):
    if np.isnan(a) or np.isnan(b) or a == b:
        return 0.0
    return abs(a - b) / max(1.0, abs(a), abs(b))


def _var_eligible(runs):
    """the reference's varI / stddevI / CVI end and have something to say: at least two runs, none NaN"""
    v = runs[3]
    return len(v) >= 2 and not np.isnan(v).any()


def _sequential(start, finish, value):
    """VarianceCorePop (statistics.c:241-249) over the non-NaN runs, MaxPop / MinPop / SpanPop (:146,176,206) with it:
    (T, sum, count, min, max)."""
    T, total, count, mn, mx = 0.0, 0.0, 0, float("nan"), float("nan")
    for a, b, x in zip(start.tolist(), finish.tolist(), value.tolist()):
        if x != x:
            continue
        length = b - a
        if count:
            old_mean, new_mean = total / count, total / (count + length)
            T += (old_mean * new_mean - new_mean * 2 * x + (count / (count + length)) * x * x) * length
        count += length
        total += length * x
        if mn != mn or x < mn:
            mn = x
        if mx != mx or x > mx:
            mx = x
    return T, total, count, mn, mx


def _closing(T, total, count, kind):
    """statistics.c:259,288-289,312-314"""
    with np.errstate(all="ignore"):
        res = np.float64(T) / np.float64(count - 1)
        if kind != "var":
            res = np.sqrt(res)
        if kind == "cv":
            res = res / (np.float64(total) / np.float64(count))
    return float(res)


CASES = [(k, op, flags) for k in range(24) for op in REDUCERS for flags in (0, 1)]


def test_enough_cases_for_the_variance_family(oracle):
    """Of the 240 combinations, those the reference's varI / stddevI / CVI can be asked about (>= 2 runs, no NaN)."""
    n = 0
    for k in range(24):
        d = random_case(9100 + k, max_len=6000).as_dict()
        n += sum(_var_eligible(oracle.reduce(d, op, flags=flags)) for op in REDUCERS for flags in (0, 1))
    assert n >= 100, n


@pytest.mark.parametrize("k", range(24))
def test_against_the_compiled_reference(oracle, H, R, k):
    """minI / maxI / span on all combinations (bit for bit; 1e-9 over the `var` reducer, whose values are held to 1e-12),
    varI / stddevI / CVI where the reference ends: bit for bit on the host path (emu), 1e-9 relative on the device (sequential
    update against ordered merge -- the tolerance fused AUC / meanI have).  Prints the largest deviation seen."""
    d = random_case(9100 + k, max_len=6000).as_dict()
    worst = 0.0
    for op in REDUCERS:
        for flags in (0, 1):
            runs = oracle.reduce(d, op, flags=flags)
            for kind in ("min", "max", "span"):
                want, got = R.run(d, kind, op, flags)[0], H.run(d, kind, op, flags)[0]
                if op in EXACT or kind == "span":
                    assert _same(got, want), (kind, op, flags, got, want)
                else:
                    assert _close(got, want), (kind, op, flags, got, want)
            if not _var_eligible(runs):
                continue
            for kind in VAR_FAMILY:
                want, got = R.run(d, kind, op, flags)[0], H.run(d, kind, op, flags)[0]
                worst = max(worst, _rel(got, want))
                if H.backend == "emu" and op in EXACT:
                    assert _same(got, want), (kind, op, flags, got, want)
                else:
                    assert _close(got, want), (kind, op, flags, got, want)
    print("moments[%s] case %d: largest deviation of varI / stddevI / CVI from the reference %.3g" % (H.backend, 9100 + k, worst))


@pytest.mark.gpu
def test_fused_means_fused(oracle, R, tmp_path_factory, monkeypatch):
    """Many small batches: one pop per BATCH, and next to nothing but counters and six doubles crossed PCIe."""
    A = _get("amd", oracle, tmp_path_factory.getbasetemp())
    monkeypatch.setenv("WTAMD_MIN_SPAN", "64")
    monkeypatch.setenv("WTAMD_BATCH_INTERVALS", "200")
    big = 0
    for k in range(24):
        d = random_case(9100 + k, max_len=6000).as_dict()
        for op in ("mean", "max"):
            for kind in ("var", "max", "span"):
                if kind == "var" and not _var_eligible(oracle.reduce(d, op)):
                    continue
                got, pops, d2h, runs = A.run(d, kind, op, 0)
                assert _close(got, R.run(d, kind, op, 0)[0]), (k, kind, op)
                if runs > 2000:
                    big += 1
                    assert pops < runs // 4, (pops, runs)
                    assert d2h < 16 * runs // 2, (d2h, runs)
    assert big >= 1, big        # (the condition above was met by some case)


def test_host_pass_through_is_the_reference(oracle, H, R, monkeypatch):
    """WTAMD_NO_FUSED_INTEGRATORS=1: one pop per run, the reference's arithmetic in the reference's order."""
    monkeypatch.setenv("WTAMD_NO_FUSED_INTEGRATORS", "1")
    for k in (0, 3, 7, 12):
        d = random_case(9100 + k, max_len=6000).as_dict()
        for op in EXACT:
            runs = oracle.reduce(d, op)
            for kind in KINDS:
                if kind in VAR_FAMILY and not _var_eligible(runs):
                    continue
                got, pops, _, _ = H.run(d, kind, op, 0)
                assert _same(got, R.run(d, kind, op, 0)[0]), (k, kind, op)
                assert pops == len(runs[0]), (k, kind, op, pops, len(runs[0]))


def _degenerate(name):
    from wiggletools_amd.runlists import RunLists
    from wiggletools_amd.textio import load_runlists
    if name == "empty":
        d = RunLists.from_lists([[[(1, 5, 1.0)]], [[(3, 9, 2.0)]]]).as_dict()
        return dict(d, seg_off=np.zeros_like(d["seg_off"]), start=d["start"][:0], finish=d["finish"][:0], value=d["value"][:0])
    if name == "one-bp":
        return RunLists.from_lists([[[(7, 8, 2.5)]]]).as_dict()
    if name == "all-zero":
        return RunLists.from_lists([[[(1, 10, 0.0), (10, 30, 0.0), (40, 55, 0.0)]], [[(5, 20, 0.0), (25, 45, 0.0)]]]).as_dict()
    G = os.path.join(HERE, "golden")
    return load_runlists([os.path.join(G, "fixedStep.wig"), os.path.join(G, "variableStep.wig")]).as_dict()


@pytest.mark.parametrize("name", ["empty", "one-bp", "all-zero", "golden"])
def test_degenerate_inputs(oracle, H, R, name):
    """An empty source, count - 1 == 0, T == 0 with mean 0, and the golden pair: whatever the reference's closing arithmetic
    gives (-0.0, NaN, inf), bit for bit, on both backends."""
    d = _degenerate(name)
    for kind in KINDS:
        want, want_pops = R.run(d, kind, "mean", 0)[:2]
        got, pops = H.run(d, kind, "mean", 0)[:2]
        print("degenerate[%s] %s %s: reference %r, got %r" % (H.backend, name, kind, want, got))
        assert _same(got, want), (name, kind, got, want)
        if name == "empty":
            assert pops == 0 and want_pops == 0


def test_nan_runs(oracle, H):
    """Over a reducer output WITH NaN runs the reference's varI / stddevI / CVI do not end (seen: still not done after 100
    pops over the runs 1, NaN, 3), so it is not run; ours end within the driver's pop cap and equal the reference's update
    applied to the non-NaN runs: bit for bit on the host path, 1e-9 on the device."""
    seen = 0
    for k in range(24):
        d = random_case(9100 + k, max_len=6000).as_dict()
        for op in REDUCERS:
            _, s, f, v = oracle.reduce(d, op)
            if not np.isnan(v).any() or (~np.isnan(v)).sum() < 2:
                continue
            seen += 1
            T, total, count, _, _ = _sequential(s, f, v)
            for kind in VAR_FAMILY:
                want, got = _closing(T, total, count, kind), H.run(d, kind, op, 0)[0]
                if H.backend == "emu" and op in EXACT:
                    assert _same(got, want), (k, op, kind, got, want)
                else:
                    assert _close(got, want), (k, op, kind, got, want)
    assert seen >= 5, seen


def _extreme(cur, vals, kind):
    for x in vals.tolist():
        if x == x and (cur != cur or (x > cur if kind == "max" else x < cur)):
            cur = x
    return cur


@pytest.mark.parametrize("pre_pops", [0, 1, 3])
def test_seek_per_region(oracle, H, pre_pops, monkeypatch):
    """`apply`'s use of the integrators: one seek per region, the moments go on across seeks (StatisticSeek / VarianceSeek,
    statistics.c:38-43,266-270).  Regions and batch sizes of test_fused_auc_seek_per_region."""
    from test_dropin import clip
    monkeypatch.setenv("WTAMD_MIN_SPAN", "64")
    monkeypatch.setenv("WTAMD_BATCH_INTERVALS", "200")
    t = random_case(8900, n_tracks=6, n_chrom=2, max_len=9000)
    d = t.as_dict()
    regions = [(0, 100, 3000), (0, 2500, 2600), (1, 1, 50), (1, 10, 4000)]
    for op in ("mean", "max"):
        clipped = [oracle.reduce(clip(t, c, s, f).as_dict(), op) for (c, s, f) in regions]
        got = H.run_seek(d, "span", regions, op=op, pre_pops=pre_pops)
        want = got[0]
        for k, (_, s, f, v) in enumerate(clipped):
            ok = ~np.isnan(v)
            want += float((f.astype(np.int64) - s)[ok].sum())
            assert got[1 + k] == want, (op, pre_pops, k, got[1 + k], want)
        for kind in ("min", "max"):
            got = H.run_seek(d, kind, regions, op=op, pre_pops=pre_pops)
            want = got[0]
            for k, (_, s, f, v) in enumerate(clipped):
                want = _extreme(want, v, kind)
                assert _same(got[1 + k], want), (kind, op, pre_pops, k, got[1 + k], want)
        # varI: the constructor's own pop absorbed whole batches and T cannot be recovered from the value -- every seek
        # re-primes cleanly and the value stays a variance
        got = H.run_seek(d, "var", regions, op=op, pre_pops=pre_pops)
        assert np.all(np.isfinite(got[1:])) and np.all(got[1:] >= 0), got


@pytest.mark.gpu
def test_bulk_door_and_python(oracle, R):
    """DeviceRuns.moments() and the six accessors over the resident output of `mean` of 100 synthetic tracks (the bench's
    generator; > 2e6 runs: every level of the device reduction) against the compiled reference over the same tracks."""
    import torch
    from wiggletools_amd import engine, synthgen
    n_tracks, clen = 100, 2_700_000
    seg, s, f, v = synthgen.device_tracks(77, [clen], n_tracks, mean_run=64.0)
    defaults = np.zeros(n_tracks)
    ts = engine.TrackSet.from_device(1, n_tracks, seg, s, f, v, defaults)
    out = ts.alloc_runs()
    n = ts.reduce("mean", out)
    assert n >= 2_000_000, n
    m = out.moments()
    d = dict(n_chrom=1, n_tracks=n_tracks, seg_off=seg, start=s.cpu().numpy(), finish=f.cpu().numpy(),
             value=v.double().cpu().numpy(), defaults=defaults)
    got = {"var": out.var(), "stddev": out.stddev(), "cv": out.cv(), "max": out.max(), "min": out.min(), "span": out.span()}
    assert m[1] == got["span"] and _close(m[0] / m[1], out.mean())
    assert out.moments().tobytes() == m.tobytes()           # the same list gives the same bits
    for kind in KINDS:
        want = R.run(d, kind, "mean", 0)[0]
        print("bulk moments, %d runs, %s: reference %r device %r (relative %.3g)" % (n, kind, want, got[kind], _rel(got[kind], want)))
        if kind in VAR_FAMILY:
            assert _close(got[kind], want), (kind, got[kind], want)
        else:
            assert _same(got[kind], want), (kind, got[kind], want)
    # an unaligned view of the same list (the scalar loads) and an odd count
    from wiggletools_amd.engine import DeviceRuns
    sub = DeviceRuns(out.start[1:n], out.finish[1:n], out.value[1:n], out.chrom_run_off)
    sub.n = n - 1
    hs, hf, hv = out.start[1:n].cpu().numpy(), out.finish[1:n].cpu().numpy(), out.value[1:n].cpu().numpy()
    T, total, count, mn, mx = _sequential(hs, hf, hv)
    m2 = sub.moments()
    assert m2[1] == count and m2[3] == mn and m2[4] == mx and _close(m2[0], total) and _close(m2[2], T), (m2, T, total, count)


def test_shard_merge_of_run_moments(oracle):
    """shard.merge_run_moments over per-chromosome moment vectors in genome order, then stats_from_moments, equals the one-pass
    sequential update over the whole genome."""
    from wiggletools_amd import shard
    from wiggletools_amd.runlists import synth
    t = synth(5, [9000, 300, 5000], mean_run=5, seed=4, gap_prob=0.2, nan_prob=0.02)
    c, s, f, v = oracle.reduce(t.as_dict(), "mean")
    rows = []
    for k in range(3):
        m = c == k
        T, total, count, mn, mx = _sequential(s[m], f[m], v[m])
        rows.append([total, float(count), T, mn, mx, 0.0])
    rows.insert(1, [0.0, 0.0, 0.0, float("nan"), float("nan"), 0.0])       # a shard without a run
    T, total, count, mn, mx = _sequential(s, f, v)
    for kind in VAR_FAMILY:
        assert _close(shard.stats_from_moments(rows, kind), _closing(T, total, count, kind)), kind
    assert shard.stats_from_moments(rows, "min") == mn and shard.stats_from_moments(rows, "max") == mx
    assert shard.stats_from_moments(rows, "span") == count
    # the NumPy merge is the host helper of the C ABI
    lib = C.CDLL(__import__("emu.build", fromlist=["build_dropin"]).build_dropin())
    lib.wtamd_moments_finish.restype = C.c_double
    lib.wtamd_moments_finish.argtypes = [C.c_void_p, C.c_int]
    acc = np.array([0.0, 0.0, 0.0, np.nan, np.nan, 0.0])
    for r in rows:
        lib.wtamd_moments_merge(acc.ctypes.data_as(C.c_void_p), np.array(r, np.float64).ctypes.data_as(C.c_void_p))
    for i, kind in enumerate(("var", "stddev", "cv", "max", "min", "span")):
        assert _same(lib.wtamd_moments_finish(acc.ctypes.data_as(C.c_void_p), i), shard.stats_from_moments(rows, kind)), kind
