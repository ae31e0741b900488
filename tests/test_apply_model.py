"""Per-region statistics (`apply`) on the CPU: the NumPy / Fraction model (tests/apply_model.py) against statistics recorded
from the compiled reference's ApplyMultiplexer (tests/golden/apply_fixtures.json); the passes of csrc/wt_apply.h run workgroup
by workgroup in shuffled order (tests/apply_emu.cpp) and the header's host sweep against the model; wtamd_apply_finish against
the model's closing arithmetic.  The same cases run on the device in tests/test_apply_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import apply_model as M
import exact

EXACT_STATS = ("AUC", "meanI", "maxI", "minI")
VAR_STATS = ("varI", "stddevI", "CVI")


@pytest.fixture(scope="module")
def fixtures():
    return M.load_fixtures()


def _reference_stream(ps, pf, pv, rs, rf, default, strict):
    """What the reference's statistics see on its buffered path (apply.c:67-100): one element per covered base pair, and in
    fill-in mode every gap as one run of the default."""
    s, f, v = [], [], []
    at = rs
    for a, b, x in zip(ps.tolist(), pf.tolist(), pv.tolist()):
        if not strict and a > at:
            s.append(at); f.append(a); v.append(default)
        s += list(range(a, b)); f += list(range(a + 1, b + 1)); v += [x] * (b - a)
        at = b
    if not strict and rf > at:
        s.append(at); f.append(rf); v.append(default)
    return np.array(s, np.int32), np.array(f, np.int32), np.array(v, np.float64)


def test_model_equals_the_compiled_reference(fixtures):
    """AUC, meanI, maxI and minI bit for bit; varI / stddevI / CVI within max(4 rel_err(sequential, exact), 1e-9) of the exact
    value, `sequential` being the run-by-run f64 update over the stream the reference's statistics saw.  The reference seeks its
    dataset to the finish of the LAST region of a buffered group (apply_model.reference_stops): where a region reaches past
    that, the recording is the definition over the dataset cut there, and the definition itself -- which clips to the region
    and to nothing else -- differs.  That departure is counted here and documented in include/wiggletools_amd.h."""
    assert len(fixtures) >= 150
    seven = cut = bitten = total = 0
    for c in fixtures:
        case, default = M.fixture_case(c)
        stops = M.reference_stops(case)
        seven += all(q in c["strict"] for q in M.STATS)
        for mode, strict in (("strict", True), ("fillin", False)):
            rec = c[mode]
            assert rec["start"] == case.rs.tolist() and rec["finish"] == case.rf.tolist(), c["name"]
            assert rec["chrom"] == np.repeat(np.arange(len(case.regions)), np.diff(case.rseg)).tolist(), c["name"]
            exp = case.expected(default, strict)
            i = 0
            for (s, f, v), (rs_, rf_) in zip(case.data, case.regions):
                for rs, rf in zip(rs_.tolist(), rf_.tolist()):
                    m = exp[i][0]
                    keep = s < stops[i]
                    cs, cf, cv = s[keep], np.minimum(f[keep], stops[i]), v[keep]
                    bites = bool((f[(s < rf)] > stops[i]).any())
                    mref = M.region_moments(cs, cf, cv, rs, rf, default, strict) if bites else m
                    w = (c["name"], mode, i, rs, rf)
                    for q in EXACT_STATS:
                        assert exact.same_bits(M.finish(mref, q), M.recorded(rec, q)[i]), w + (q,)
                    if "varI" in rec:
                        ps, pf, pv = M.pieces(cs, cf, cv, rs, rf)
                        T, total_, count = exact.seq_moments(*_reference_stream(ps, pf, pv, rs, rf, default, strict))[:3]
                        seq = np.array([total_, count, T, 0.0, 0.0, 0.0])
                        for q in VAR_STATS:
                            e = M.finish(mref, q)
                            assert exact.rel_err(M.recorded(rec, q)[i], e) <= max(4 * exact.rel_err(M.finish(seq, q), e), 1e-9), w + (q,)
                    cut += bites and not all(exact.same_bits(M.finish(mref, q), M.finish(m, q)) for q in EXACT_STATS)
                    bitten += bites
                    total += 1
                    i += 1
    assert seven >= 0.8 * len(fixtures), seven
    assert 0 < cut <= bitten < total, (cut, bitten, total)      # the recordings do hold the departure, and only where the seek bites


def test_finish_is_the_model_closing_arithmetic(fixtures):
    from wiggletools_amd import _lib
    from wiggletools_amd.csrc import build as hip_build
    hip_build.build()                               # (a host function of the library: no GPU needed)
    L = C.CDLL(_lib.LIB_PATH)
    L.wtamd_apply_finish.restype = C.c_double
    L.wtamd_apply_finish.argtypes = [C.c_void_p, C.c_int]
    rows = [np.array([0.0, 0.0, 0.0, np.nan, np.nan, 0.0]), np.array([2.5, 1.0, 0.0, 2.5, 2.5, 1.0]), np.array([-0.0, 4.0, 0.0, -0.0, 0.0, 4.0])]
    for c in fixtures[:20]:
        case, default = M.fixture_case(c)
        rows += [m for m, _, _ in case.expected(default, False)]
    for m in rows:
        m = np.ascontiguousarray(m)
        for k, q in enumerate(M.STATS):
            assert exact.same_bits(L.wtamd_apply_finish(m.ctypes.data, k), M.finish(m, q)), (m.tolist(), q)
        assert np.isnan(L.wtamd_apply_finish(m.ctypes.data, 7)) and np.isnan(L.wtamd_apply_finish(m.ctypes.data, -1))


def _check_emu(case, what):
    for default in M.DEFAULTS:
        for strict in (True, False):
            got = []
            for k, (order, dt) in enumerate(((0, np.float64), (2, np.float32), (2, np.float64))):
                rc, out = M.emu_case(case, default, strict, dt, order=order, seed=17 + k)
                assert rc == M.OK, what
                M.check(case, out, default, strict, what)
                got.append(out)
            assert M.same_rows(got[0], got[1]) and M.same_rows(got[1], got[2]), what       # two shuffles, either width: the same bits
            rc, host = M.host_sweep(case, default, strict)
            assert rc == M.OK
            M.check(case, host, default, strict, what + " host sweep")


def test_emulated_passes_and_host_sweep_on_the_fixtures(fixtures):
    for c in fixtures:
        case, default = M.fixture_case(c)
        for strict in (True, False):
            for order in (0, 2):
                rc, out = M.emu_case(case, default, strict, np.float32, order=order, seed=3)
                assert rc == M.OK
                M.check(case, out, default, strict, c["name"])
            rc, host = M.host_sweep(case, default, strict)
            assert rc == M.OK
            M.check(case, host, default, strict, c["name"] + " host sweep")
    # all of them in one call: some 300 segments
    one, _ = M.all_fixtures_in_one(fixtures)
    _check_emu(one, "all")


SEAMS = M.seam_cases()


@pytest.mark.parametrize("name", sorted(SEAMS))
def test_emulated_passes_at_the_seams(name):
    _check_emu(SEAMS[name], name)


def test_seam_cases_are_what_they_claim():
    c = M.constants()
    S, CH, W, T = c["SMALL"], c["CHUNK"], c["WINDOW"], c["TILE"]
    assert S < CH and W >= S and T % 256 == 0
    for n in (S - 1, S, S + 1, CH - 1, CH, CH + 1, 3 * CH + 5):
        for sfx in ("", "_float"):
            k = SEAMS["runs%d%s" % (n, sfx)]
            ps, pf, _ = M.pieces(k.s, k.f, k.v, int(k.rs[0]), int(k.rf[0]))
            assert len(ps) == n and k.exact_sum == (sfx == "")
            assert ps[0] > k.s[7] or k.f[7] - k.s[7] == 1            # clipped in its first run where that run is longer than 1 bp
    for n in (T - 1, T, T + 1, 3 * T + 5):
        k = SEAMS["regions%d" % n]
        under = np.array([len(M.pieces(k.s, k.f, k.v, int(a), int(b))[0]) for a, b in zip(k.rs, k.rf)])
        assert len(k.rs) == n and (under > S).sum() >= 5 and (under <= S).sum() > n - 20 and (under == 0).any()
    for w in (W, W + 1):
        k = SEAMS["window%d" % w]
        lo = np.searchsorted(k.f, k.rs[0], side="right")
        hi = np.searchsorted(k.s, k.rf.max(), side="left")
        assert hi - lo == w and len(k.rs) <= T
    k = SEAMS["segments"]
    assert len(k.rs) < T
    kinds = {(len(d[0]) > 0, len(r[0]) > 0) for d, r in zip(k.data, k.regions)}
    assert kinds == {(True, True), (True, False), (False, True), (False, False)}
    # the edges, spelled out: strict, then fill-in with 1.5
    k = SEAMS["edges"]
    st = {(int(a), int(b)): m for a, b, (m, _, _) in zip(k.rs, k.rf, k.expected(0.0, True))}
    fi = {(int(a), int(b)): m for a, b, (m, _, _) in zip(k.rs, k.rf, k.expected(1.5, False))}
    assert st[(1, 10)].tolist()[:3] == [0.0, 0.0, 0.0] and np.isnan(st[(1, 10)][3]) and st[(1, 10)][5] == 0
    assert st[(1, 11)].tolist() == [1.0, 1.0, 0.0, 1.0, 1.0, 1.0]                   # one base pair of the first run
    assert st[(12, 18)].tolist() == [6.0, 6.0, 0.0, 1.0, 1.0, 6.0]                  # a single run clipped on both ends
    assert st[(20, 25)].tolist()[:2] == [0.0, 0.0] and st[(20, 25)][5] == 5         # a NaN run: covered, not in the span
    assert fi[(20, 30)].tolist() == [7.5, 5.0, 0.0, 1.5, 1.5, 5.0]                  # ... and the gap behind it filled
    assert st[(60, 61)][5] == 0 and fi[(60, 900)].tolist() == [1260.0, 840.0, 0.0, 1.5, 1.5, 0.0]
    m = st[(30, 41)]
    assert exact.same_bits(m[3], -0.0) and exact.same_bits(m[4], -0.0)              # the first of -0.0 and 0.0 is both extremes
    assert fi[(5, 70)][1] == 60 and fi[(5, 70)][5] == 36                            # 65 bp, 5 of them under the NaN run


def test_a_region_alone_equals_the_region_inside_the_full_call():
    rng = np.random.default_rng(5)
    for name in ("regions%d" % (3 * M.constants()["TILE"] + 5), "runs%d_float" % (3 * M.constants()["CHUNK"] + 5), "segments_many", "window%d" % M.constants()["WINDOW"]):
        case = SEAMS[name]
        for default, strict in ((0.0, True), (1.5, False)):
            rc, full = M.emu_case(case, default, strict, np.float32, order=2, seed=1)
            assert rc == M.OK
            picks = np.unique(np.concatenate([[0, len(case.rs) - 1], rng.integers(0, len(case.rs), 12)]))
            for i in picks:
                rc, alone = M.emu_case(case.subset([i]), default, strict, np.float32, order=2, seed=2)
                assert rc == M.OK and M.same_rows(alone, full[i:i + 1]), (name, i)
            # ... and a third of the regions, which moves every one of them to another lane and tile
            idx = np.arange(0, len(case.rs), 3)
            rc, part = M.emu_case(case.subset(idx), default, strict, np.float32, order=2, seed=3)
            assert rc == M.OK and M.same_rows(part, full[idx]), name


def test_emulated_refusals_leave_the_output_untouched():
    case = SEAMS["segments"]
    seg, s, f, v, rseg, rs, rf = case.seg, case.s, case.f, case.v, case.rseg, case.rs, case.rf

    def door(s_=s, f_=f, rs_=rs, rf_=rf, flags=None):
        rc, out = M.emu_apply(seg, s_, f_, v, rseg, rs_, rf_, 0.0, True, order=2, seed=9, flags=flags)
        return rc, bool((out == -1.0).all())
    assert door()[0] == M.OK
    s2 = s.copy(); s2[5], s2[6] = s[6], s[5]                          # dataset not sorted
    f3 = f.copy(); f3[9] = s[9]                                       # an empty dataset run
    f4 = f.copy(); f4[3] = s[4] + 1                                   # dataset runs 3 and 4 overlap
    rs2 = rs.copy(); rs2[2], rs2[3] = max(rs[2], rs[3]) + 1, min(rs[2], rs[3])
    rf2 = np.maximum(rf, rs2 + 1)                                     # regions not sorted
    rf3 = rf.copy(); rf3[4] = rs[4]                                   # an empty region
    assert s[4] > s[3] and rs2[2] > rs2[3]
    s5 = s.copy(); s5[0] = -1                                         # a negative start, either side
    rs5 = rs.copy(); rs5[0] = -1
    for kw in (dict(s_=s2), dict(f_=f3), dict(f_=f4), dict(rs_=rs2, rf_=rf2), dict(rf_=rf3), dict(flags=2), dict(s_=s5), dict(rs_=rs5)):
        assert door(**kw) == (M.ERR_ARG, True), sorted(kw)
    # a start below the one in front of it at a segment boundary is fine, and so are regions that overlap
    assert s[seg[2]] < s[seg[2] - 1] and (rs[1:] < rf[:-1]).any()


def test_dropin_apply_multiplexer_on_the_host(fixtures):
    """wtamd_ApplyMultiplexer in the emulated drop-in library (no HIP unit: the weak reference to the device door is null and
    the Multiplexer sweeps on the host): by pop, under SelectReduction, after a seek, over a MeanReduction."""
    import apply_dropin
    from emu import build as emu_build
    apply_dropin.check_dropin(apply_dropin.DropIn(emu_build.build_dropin()), fixtures)
