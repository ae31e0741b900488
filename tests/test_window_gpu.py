"""The window operators on the device (csrc/wt_window.hip: wtamd_runs_bin, wtamd_runs_smooth) against every value recorded from
the compiled reference and against the per-pop Fraction model of tests/window_model.py, which tests/test_window_model.py pins
to those recordings: bit for bit wherever the values are multiples of 1/8 (every sum is then exact), within the derived bounds
for float values.  The seam sizes come from the header's constants (window_model.constants)."""
import functools

import numpy as np
import pytest

import window_model as M

pytestmark = pytest.mark.gpu

BIN_SEAMS = M.bin_seams()
SMOOTH_SEAMS = M.smooth_seams()


def _rl(case, dt, default=0.0):
    from wiggletools_amd.runlists import RunLists
    return RunLists(len(case.seg) - 1, 1, case.seg, case.s, case.f, case.v.astype(dt), [default])


def _bin(case, w, default=0.0, dt=np.float32, **kw):
    from wiggletools_amd import engine
    return engine._window_door(_rl(case, dt), w, default, **kw)


def _smooth(case, w, dt=np.float32, **kw):
    from wiggletools_amd import engine
    return engine._window_door(_rl(case, dt), w, None, **kw)


def _same_out(a, b, n):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1][:n], b[1][:n]) and np.array_equal(a[2][:n], b[2][:n]) and M.same_bits(a[3][:n], b[3][:n])


def _check_bin(case, w, default, what, model=None):
    model = M.bin(case.chroms, w, default) if model is None else model
    outs = []
    for dt in (np.float32, np.float64):
        rc, n, got = _bin(case, w, default, dt)
        assert rc == M.OK and n == len(model), what
        M.check_exact(got, model, len(case.chroms), what)
        outs.append(got)
    assert _same_out(outs[0], outs[1], len(model)), what                # the same values in either width: the same bits
    return outs[0]


def _check_smooth(case, w, what, model=None):
    model = M.smooth(case.chroms, w) if model is None else model
    outs = []
    for dt in (np.float32, np.float64):
        rc, n, got = _smooth(case, w, dt)
        assert rc == M.OK and n == len(model), what
        M.check_exact(got, model, len(case.chroms), what)
        outs.append(got)
    assert _same_out(outs[0], outs[1], len(model)), what
    return outs[0]


def _recorded_as_model(rec):
    return [(c, s, f, M.Term(v, 0, 0)) for c, s, f, v in M.recorded(rec)]


def test_fixtures_case_by_case_against_the_recordings():
    for c in M.load_fixtures():
        case, default, w = M.fixture_case(c)
        _check_bin(case, w, default, (c["name"], "bin"), _recorded_as_model(c["bin"]))
        _check_smooth(case, w, (c["name"], "smooth"), _recorded_as_model(c["smooth"]))


@functools.lru_cache(None)
def _all_in_one():
    chroms = []
    for c in M.load_fixtures():
        chroms += M.fixture_case(c)[0].chroms
    return M.Case(chroms)


def test_fixtures_all_in_one_call():
    one = _all_in_one()
    _check_bin(one, 7, 1.5, "all bin")
    _check_smooth(one, 10, "all smooth")


@pytest.mark.parametrize("name", sorted(BIN_SEAMS))
def test_bin_seams(name):
    """w = 2; a run over 3 TILE + 5 bins; SMALL - 1 .. SMALL + 2 and WAVE x SMALL - 1 .. + 1 runs in a bin; a window of exactly
    WINDOW and WINDOW + 1 runs under one tile; empty segments on either side; a first start of 1; NaN runs."""
    case, w = BIN_SEAMS[name]
    for default in M.DEFAULTS:
        got = _check_bin(case, w, default, name)
    rc, n, emu = M.emu_bin(case, w, M.DEFAULTS[-1], np.float32, order=2, seed=4)
    assert rc == M.OK and _same_out(emu, got, n), name              # the emulated passes in shuffled order give the device's bits


@pytest.mark.parametrize("name", sorted(SMOOTH_SEAMS))
def test_smooth_seams(name):
    """w of 2, 3 and 4099; an extent of STRIP - 1 .. 3 STRIP + 5 and around a workgroup's 256 strips; a chromosome of 1 .. w + 1
    positions; a first start of 1, h and h + 1; a last finish <= h; a NaN run entering, leaving and sitting in the trailing phase;
    a gap longer than w; empty segments on either side."""
    case, w = SMOOTH_SEAMS[name]
    got = _check_smooth(case, w, name)
    rc, n, emu = M.emu_smooth(case, w, np.float32, order=2, seed=4)
    assert rc == M.OK and _same_out(emu, got, n), name


def test_a_segment_alone_equals_the_segment_inside_the_full_call():
    one = _all_in_one()
    rng = np.random.default_rng(5)
    rc, n, (bseg, bs, bf, bv) = _bin(one, 7, 1.5)
    rc2, n2, (sseg, ss, sf, sv) = _smooth(one, 10)
    assert rc == M.OK and rc2 == M.OK
    for g in rng.integers(0, len(one.chroms), 8):
        rc, k, (_, s, f, v) = _bin(one.only(g), 7, 1.5)
        a = int(bseg[g])
        assert rc == M.OK and k == bseg[g + 1] - a and np.array_equal(s[:k], bs[a:a + k]) and M.same_bits(v[:k], bv[a:a + k]), g
        rc, k, (_, s, f, v) = _smooth(one.only(g), 10)
        a = int(sseg[g])
        assert rc == M.OK and k == sseg[g + 1] - a and np.array_equal(s[:k], ss[a:a + k]) and M.same_bits(v[:k], sv[a:a + k]), g


def test_a_clipped_smooth_is_the_slice_of_the_whole():
    c = M.constants()
    for name, clips in (("extent%d" % (c["STRIP"] * 256 + 1), ((1, 60), (47, 48), (60, c["STRIP"] * 256 + 70), (5000, 6000), (3, 2 ** 31 - 1))),
                        ("segments", ((1, 9), (100, 517), (30, 31)))):
        case, w = SMOOTH_SEAMS[name]
        rc, n, (oseg, os_, of, ov) = _smooth(case, w)
        assert rc == M.OK
        seg_of = np.repeat(np.arange(len(oseg) - 1), np.diff(oseg))
        for lo, hi in clips:
            rc, k, (cseg, cs, cf, cv) = _smooth(case, w, clip=(lo, hi))
            keep = (os_[:n] >= lo) & (os_[:n] < hi)
            assert rc == M.OK and k == keep.sum(), (name, lo, hi)
            assert np.array_equal(cs[:k], os_[:n][keep]) and np.array_equal(cf[:k], of[:n][keep]) and M.same_bits(cv[:k], ov[:n][keep]), (name, lo, hi)
            assert np.array_equal(np.diff(cseg), np.bincount(seg_of[keep], minlength=len(oseg) - 1)), (name, lo, hi)


def test_two_thousand_float_runs_within_the_derived_bounds():
    case = M.float_case()
    for w in (3, 10, 1000):
        rc, n, got = _bin(case, w, 1.5)
        assert rc == M.OK
        M.check_bin_bound(got, M.bin(case.chroms, w, 1.5), 1, ("float bin", w))
        rc, k, emu = M.emu_bin(case, w, 1.5, np.float32, order=2, seed=9)
        assert _same_out(emu, got, n)
    for w in (3, 10, 100):
        rc, n, got = _smooth(case, w)
        assert rc == M.OK
        M.check_smooth_bound(got, M.smooth(case.chroms, w), case, w, ("float smooth", w))
        rc, k, emu = M.emu_smooth(case, w, np.float32, order=2, seed=9)
        assert _same_out(emu, got, n)


def test_refusals_leave_the_output_untouched():
    from wiggletools_amd import engine
    case, w = BIN_SEAMS["segments"]
    untouched = lambda got: (got[1] == -1).all() and (got[2] == -1).all() and (got[3] == -1.0).all()      # noqa: E731
    for what, bad, width in M.refusals(case):
        rc, n, got = _bin(bad, width, 1.5, capacity=4000)
        assert rc == M.ERR_ARG and untouched(got), what
        rc, n, got = _smooth(bad, width, capacity=4000)
        assert rc == M.ERR_ARG and untouched(got), what
    need = len(M.bin(case.chroms, w, 0.0))
    rc, n, got = _bin(case, w, 0.0, capacity=need - 1)
    assert rc == M.ERR_CAPACITY and n == need and untouched(got)
    need = len(M.smooth(case.chroms, w))
    rc, n, got = _smooth(case, w, capacity=need - 1)
    assert rc == M.ERR_CAPACITY and n == need and untouched(got)
    with pytest.raises(Exception):
        engine.bin_runlists(_rl(M.refusals(case)[4][1], np.float32), 7)
    out = engine.smooth_runlists(_rl(case, np.float32, 1.5), w)
    assert out.seg_off[-1] == need and out.defaults[0] == 1.5
    assert engine.bin_runlists(_rl(case, np.float32, 1.5), w).defaults[0] == 1.5 * w


def test_dropin_window_iterators(monkeypatch):
    """wtamd_BinIterator and wtamd_SmoothIterator in the product: every recorded case by pop through the device doors and again
    with WTAMD_NO_DEVICE_WINDOW=1 (the same bits), against the recording; in blocks, after a seek, under a SumReduction of this
    library, over an overlapping child and over a chromosome that starts below 1."""
    import window_dropin
    from wiggletools_amd import _lib
    _lib.lib()
    window_dropin.check_dropin(window_dropin.DropIn(_lib.LIB_PATH), M.load_fixtures(), setenv=monkeypatch.setenv)
