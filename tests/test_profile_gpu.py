"""Region profiles on the device (csrc/wt_profile.hip: wtamd_runs_profile) against the per-base-pair Fraction model of
tests/profile_model.py, which tests/test_profile_model.py pins to rows recorded from the compiled reference: bit for bit where
a bin is exact (every term a multiple of 2^-10, sum of |terms| < 2^40), within (k + 2) 2^-52 sum of |terms| elsewhere.  The seam
sizes come from the header's constants (profile_model.constants)."""
import numpy as np
import pytest

import apply_model as AM
import profile_model as M

pytestmark = pytest.mark.gpu

ROUNDING = M.rounding_cases()
REGIMES = M.regime_cases()


def _rl(seg, s, f, v=None):
    from wiggletools_amd.runlists import RunLists
    return RunLists(len(seg) - 1, 1, seg, s, f, np.ones(len(s), np.float32) if v is None else v)


def _door(case, W, default=0.0, dt=np.float64, **kw):
    from wiggletools_amd import engine
    return engine._profile_door(_rl(case.seg, case.s, case.f, case.values(dt)), _rl(case.rseg, case.rs, case.rf), W, default, **kw)


def _check(case, W, what, defaults=M.DEFAULTS, sums=True):
    exp = M.Expected(case)
    rows = None
    for default in defaults:
        got = []
        for dt in (np.float32, np.float64):
            rc, out = _door(case, W, default, dt)
            assert rc == M.OK, what
            got.append(out)
        exp.check(got[0], W, default, what)
        assert M.same_rows(got[0], got[1]), what                    # the same values in either width: the same bits
        rows = got[0]
        if sums:
            rc, out = _door(case, W, default, np.float32, sum=True)
            assert rc == M.OK, what
            exp.check(out, W, default, what + " sum", sum_mode=True)
    return rows                                                     # (of the last default)


def test_fixtures_in_one_call_and_case_by_case():
    cases = M.load_fixtures()
    one, _ = AM.all_fixtures_in_one(cases)
    for W in (3, 64):
        _check(one, W, "all", defaults=(1.5,))
    for c in cases:
        case, default, W = M.fixture_case(c)
        rows = _check(case, W, c["name"], defaults=(default,))
        # against the recording itself, wherever the reference's group seek did not cut the dataset short
        stops, rec = AM.reference_stops(case), M.recorded_rows(c)
        seg_of = np.repeat(np.arange(len(case.regions)), np.diff(case.rseg))
        bins = M.Expected(case).rows(W, default)
        for i in range(len(case.rs)):
            s, f, _ = case.data[seg_of[i]]
            if (f[s < case.rf[i]] > stops[i]).any():
                continue
            for j in range(W):
                if bins[i][j].exact:
                    assert rows[i][j] == rec[i][j], (c["name"], i, j)


@pytest.mark.parametrize("name", sorted(ROUNDING))
def test_rounding_seams(name):
    """L == 2W (a tie at every odd position), L == W, L == W +- 1, L == 2W +- 1, W == 1, L == 1, L = 999 983 with W = 1000,
    W = 4099 with L = 3, and the two worked examples -- defaults 0, 1.5 and NaN, f32 and f64, per region and summed."""
    case, W = ROUNDING[name]
    _check(case, W, name)


@pytest.mark.parametrize("name", sorted(REGIMES))
def test_regime_seams(name):
    """SMALL - 1 .. SMALL + 2, WAVE - 1 .. WAVE + 1 and SMALL x WAVE - 1 .. 3 SMALL x WAVE + 5 runs under one bin; T - 1 ..
    3T + 5 regions; a window of exactly WINDOW and WINDOW + 1 runs under one tile; several segments in one tile with empty ones
    on either side; a region with no data, one inside one run, gaps over several bins, a gap into the dropped tail, NaN runs."""
    case, W = REGIMES[name]
    _check(case, W, name, defaults=(1.5,) if name.startswith("regions") else M.DEFAULTS)


def test_two_thousand_float_runs_and_one_region_over_everything():
    case = M.float_case()
    for W in (1, 5, 300):
        _check(case, W, "float", defaults=(1.5,))


def test_a_region_alone_equals_the_region_inside_the_full_call():
    rng = np.random.default_rng(5)
    c = M.constants()
    for name in ("regions%d" % (3 * c["TILE"] + 5), "bin%d_float" % (3 * c["SMALL"] * c["WAVE"] + 5), "segments", "window%d" % c["WINDOW"]):
        case, W = REGIMES[name]
        rc, full = _door(case, W, 1.5, np.float32)
        assert rc == M.OK
        for i in np.unique(np.concatenate([[0, len(case.rs) - 1], rng.integers(0, len(case.rs), 6)])):
            rc, alone = _door(case.subset([i]), W, 1.5, np.float32)
            assert rc == M.OK and M.same_rows(alone, full[i:i + 1]), (name, i)
        idx = np.arange(0, len(case.rs), 3)
        rc, part = _door(case.subset(idx), W, 1.5, np.float32)
        assert rc == M.OK and M.same_rows(part, full[idx]), name
        # ... and the emulated passes in shuffled order give the device's bits, per region and summed
        rc, emu = M.emu_case(case, W, 1.5, 0, np.float32, order=2, seed=4)
        assert rc == M.OK and M.same_rows(emu, full), name
        rc, dev_sum = _door(case, W, 1.5, np.float32, sum=True)
        rc2, emu_sum = M.emu_case(case, W, 1.5, M.SUM, np.float32, order=2, seed=4)
        assert rc == M.OK and rc2 == M.OK and M.same_rows(emu_sum, dev_sum), name


def test_the_sum_has_the_same_bits_whatever_the_batch(monkeypatch):
    case = M.float_case()
    exp = M.Expected(case)
    for W in (1, 5):
        monkeypatch.delenv("WTAMD_PROFILE_BATCH", raising=False)
        rc, whole = _door(case, W, 1.5, sum=True)
        assert rc == M.OK
        exp.check(whole, W, 1.5, "float sum", sum_mode=True)
        rc, rows_whole = _door(case, W, 1.5)
        for batch in (1, 4, 64):
            monkeypatch.setenv("WTAMD_PROFILE_BATCH", str(batch))
            rc, out = _door(case, W, 1.5, sum=True)
            assert rc == M.OK and M.same_rows(out, whole), (W, batch)
            rc, rows = _door(case, W, 1.5)
            assert rc == M.OK and M.same_rows(rows, rows_whole), (W, batch)
        # R = batch - 1, batch and batch + 1 regions
        for n in (63, 64, 65):
            sub = case.subset(np.arange(n))
            monkeypatch.setenv("WTAMD_PROFILE_BATCH", "64")
            rc, a = _door(sub, W, 1.5, sum=True)
            monkeypatch.delenv("WTAMD_PROFILE_BATCH")
            rc2, b = _door(sub, W, 1.5, sum=True)
            assert rc == M.OK and rc2 == M.OK and M.same_rows(a, b), (W, n)
            M.Expected(sub).check(a, W, 1.5, "float sum %d" % n, sum_mode=True)


def test_refusals_leave_the_output_untouched():
    from wiggletools_amd import engine
    case, W = REGIMES["segments"]
    assert _door(case, W, 0.0, np.float32)[0] == M.OK
    for what, kw in M.refusals(case):
        kw = dict(kw)
        w, flags = kw.pop("W", W), kw.pop("flags", None)
        rc, out = _door(M.altered(case, **kw), w, 0.0, np.float32, flags=flags)
        assert rc == M.ERR_ARG and (out == -1.0).all(), what
    bad = M.altered(case, **dict(M.refusals(case))["overlapping dataset"])
    with pytest.raises(Exception):
        engine.profile_runlists(_rl(bad.seg, bad.s, bad.f, bad.values(np.float32)), _rl(bad.rseg, bad.rs, bad.rf), W)


def test_dropin_profile_multiplexer(monkeypatch):
    """wtamd_ProfileMultiplexer in the product: every recorded case by pop through the device door and again with
    WTAMD_NO_DEVICE_PROFILE=1 (the same bits), against the recording and the model; under SelectReduction, after a
    seekMultiplexer, and with a MeanReduction of this library as the dataset."""
    import profile_dropin
    from wiggletools_amd import _lib
    _lib.lib()
    profile_dropin.check_dropin(profile_dropin.DropIn(_lib.LIB_PATH), M.load_fixtures(), setenv=monkeypatch.setenv)
