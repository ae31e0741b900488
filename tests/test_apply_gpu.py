"""Per-region statistics on the device (csrc/wt_apply.hip: wtamd_runs_apply) against the NumPy / Fraction model of
tests/apply_model.py, which tests/test_apply_model.py pins to statistics recorded from the compiled reference.  span, covered,
min and max bit for bit, the sum bit for bit where the values are k / 8 and within the model's rounding bound elsewhere, T
within max(4 rel_err(sequential, exact), 1e-9).  The seam sizes come from the header's constants (apply_model.constants)."""
import numpy as np
import pytest

import apply_model as M
import exact

pytestmark = pytest.mark.gpu

SEAMS = M.seam_cases()


def _rl(seg, s, f, v=None):
    from wiggletools_amd.runlists import RunLists
    return RunLists(len(seg) - 1, 1, seg, s, f, np.ones(len(s), np.float32) if v is None else v)


def _door(case, default=0.0, strict=True, dt=np.float64, **kw):
    from wiggletools_amd import engine
    return engine._apply_door(_rl(case.seg, case.s, case.f, case.values(dt)), _rl(case.rseg, case.rs, case.rf), default, strict, **kw)


def _check(case, what, defaults=M.DEFAULTS):
    rows = {}
    for default in defaults:
        for strict in (True, False):
            got = []
            for dt in (np.float32, np.float64):
                rc, out = _door(case, default, strict, dt)
                assert rc == M.OK, what
                M.check(case, out, default, strict, what)
                got.append(out)
            assert M.same_rows(got[0], got[1]), what                # the same values in either width: the same bits
            rows[strict] = got[0]
    return rows                                                     # (of the last default)


def test_fixtures_in_one_call_and_case_by_case():
    from wiggletools_amd import engine
    cases = M.load_fixtures()
    one, _ = M.all_fixtures_in_one(cases)
    _check(one, "all")
    for c in cases:
        case, default = M.fixture_case(c)
        rows = _check(case, c["name"], defaults=(default,))
        # against the recording itself, wherever the reference's group seek did not cut the dataset short
        stops = M.reference_stops(case)
        for mode, strict in (("strict", True), ("fillin", False)):
            seg_of = np.repeat(np.arange(len(case.regions)), np.diff(case.rseg))
            for i in range(len(case.rs)):
                s, f, _ = case.data[seg_of[i]]
                if (f[s < case.rf[i]] > stops[i]).any():
                    continue
                for q in ("AUC", "meanI", "maxI", "minI"):
                    assert exact.same_bits(engine.apply_finish(rows[strict][i], q), M.recorded(c[mode], q)[i]), (c["name"], mode, i, q)


@pytest.mark.parametrize("name", sorted(SEAMS))
def test_seams(name):
    """SMALL - 1 .. SMALL + 1 and CHUNK - 1 .. 3 CHUNK + 5 runs under a region whose first and last run are clipped; T - 1 ..
    3T + 5 regions; a window of W and of W + 1 runs under one tile; several segments in one tile, empty ones on either side; a
    single run clipped on both ends, touching edges, NaN runs, -0.0 -- defaults 0, 1.5 and NaN, strict and fill-in, f32 and f64."""
    _check(SEAMS[name], name)


def test_forty_thousand_runs_five_thousand_regions_and_one_over_everything():
    case = M.mid_size()
    assert len(case.s) == 40000 and len(case.rs) == 5001 and case.rs[0] <= case.s[0] and case.rf[0] >= case.f[-1]
    _check(case, "mid", defaults=(1.5,))


def test_a_region_alone_equals_the_region_inside_the_full_call():
    rng = np.random.default_rng(5)
    c = M.constants()
    for name in ("regions%d" % (3 * c["TILE"] + 5), "runs%d_float" % (3 * c["CHUNK"] + 5), "segments_many"):
        case = SEAMS[name]
        for default, strict in ((0.0, True), (1.5, False)):
            rc, full = _door(case, default, strict, np.float32)
            assert rc == M.OK
            for i in np.unique(np.concatenate([[0, len(case.rs) - 1], rng.integers(0, len(case.rs), 6)])):
                rc, alone = _door(case.subset([i]), default, strict, np.float32)
                assert rc == M.OK and M.same_rows(alone, full[i:i + 1]), (name, i)
            idx = np.arange(0, len(case.rs), 3)
            rc, part = _door(case.subset(idx), default, strict, np.float32)
            assert rc == M.OK and M.same_rows(part, full[idx]), name
            # ... and the emulated passes give the device's bits
            rc, emu = M.emu_case(case, default, strict, np.float32, order=2, seed=4)
            assert rc == M.OK and M.same_rows(emu, full), name


def test_refusals_leave_the_output_untouched():
    from wiggletools_amd import engine
    case = SEAMS["segments"]
    seg, s, f, rseg, rs, rf = case.seg, case.s, case.f, case.rseg, case.rs, case.rf
    v = case.values(np.float32)

    def door(s_=s, f_=f, rs_=rs, rf_=rf, flags=None):
        rc, out = engine._apply_door(_rl(seg, s_, f_, v), _rl(rseg, rs_, rf_), 0.0, True, flags=flags)
        return rc, bool((out == -1.0).all())
    assert door()[0] == M.OK
    s2 = s.copy(); s2[5], s2[6] = s[6], s[5]
    f3 = f.copy(); f3[9] = s[9]
    f4 = f.copy(); f4[3] = s[4] + 1
    rs2 = rs.copy(); rs2[2], rs2[3] = max(rs[2], rs[3]) + 1, min(rs[2], rs[3])
    rf2 = np.maximum(rf, rs2 + 1)
    rf3 = rf.copy(); rf3[4] = rs[4]
    s5 = s.copy(); s5[0] = -1                                         # a negative start, either side
    rs5 = rs.copy(); rs5[0] = -1
    for kw in (dict(s_=s2), dict(f_=f3), dict(f_=f4), dict(rs_=rs2, rf_=rf2), dict(rf_=rf3), dict(flags=2), dict(s_=s5), dict(rs_=rs5)):
        assert door(**kw) == (M.ERR_ARG, True), sorted(kw)
    with pytest.raises(Exception):
        engine.apply_runlists(_rl(seg, s, f4, v), _rl(rseg, rs, rf))


def test_dropin_apply_multiplexer(monkeypatch):
    """wtamd_ApplyMultiplexer in the product: every recorded case by pop through the device door and again with
    WTAMD_NO_DEVICE_APPLY=1 (the same bits), against the recording and the model; under SelectReduction, after a
    seekMultiplexer, and with a MeanReduction of this library as the dataset."""
    import apply_dropin
    from wiggletools_amd import _lib
    _lib.lib()
    apply_dropin.check_dropin(apply_dropin.DropIn(_lib.LIB_PATH), M.load_fixtures(), setenv=monkeypatch.setenv)
