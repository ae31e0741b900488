"""The region operators on the device (csrc/wt_region.hip: wtamd_runs_region, wtamd_RegionIterator) against the NumPy model of
tests/region_model.py, which tests/test_region_model.py pins to output recorded from the compiled reference.  Every comparison
is exact: coordinates, offsets and value bits.  The seam sizes come from the header's constants (region_model.constants)."""
import numpy as np
import pytest

import region_dropin
import region_model as M

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_CAPACITY = 0, 1, 3
OPS = sorted(M.OPS, key=M.OPS.get)
SEAMS = M.seam_cases()


def _rl(seg, s, f, v=None):
    from wiggletools_amd.runlists import RunLists
    return RunLists(len(seg) - 1, 1, seg, s, f, np.ones(len(s), np.float32) if v is None else v)


def _check(op, seg, s, f, v, mseg, ms, mf, what=""):
    from wiggletools_amd import engine
    got = engine.region_runlists(op, _rl(seg, s, f, v), _rl(mseg, ms, mf))
    exp = M.segmented(op, seg, s, f, v, mseg, ms, mf)
    assert np.array_equal(got.seg_off, exp[0]), (what, op)
    assert np.array_equal(got.start, exp[1]) and np.array_equal(got.finish, exp[2]) and M.same_bits(got.value, exp[3]), (what, op)


def test_fixtures_in_one_call_and_case_by_case():
    cases = region_dropin.load_fixtures()
    for op in OPS:
        seg, s, f, v, mseg, ms, mf = region_dropin.all_in_one(cases, op)
        _check(op, seg, s, f, v, mseg, ms, mf, "all")
        _check(op, seg, s, f, v.astype(np.float32), mseg, ms, mf, "all f32")
    from wiggletools_amd import engine
    for c in cases[:8]:
        seg, s, f, v, mseg, ms, mf = region_dropin.case_arrays(c)
        for op in OPS:
            if op not in c:
                continue
            _check(op, seg, s, f, v, mseg, ms, mf, c["name"])
            # against the recording itself
            got = engine.region_runlists(op, _rl(seg, s, f, v), _rl(mseg, ms, mf))
            rec = c[op]
            assert np.array_equal(got.start, rec["start"]) and np.array_equal(got.finish, rec["finish"]), (c["name"], op)
            assert M.same_bits(got.value, region_dropin.recorded_values(rec)), (c["name"], op)


@pytest.mark.parametrize("name", sorted(SEAMS))
def test_seams(name):
    """T - 1, T, T + 1 and 3T + 5 source runs; a mask window of W and of W + 1 groups under one tile; a trim run that ends
    its tile and meets 2T + 3 groups; several segments in one tile, empty ones among them; strictness; the nearest quirks --
    with NaN (payload), -0.0 and denormal values, f32 and f64 (tests/region_model.py)."""
    src, mask = SEAMS[name]
    seg, s, f = M.flat(src)
    mseg, ms, mf = M.flat(mask)
    for op in OPS:
        if op == "trim" and M.overlaps_itself(seg, s, f):
            continue                        # refused: test_refusals
        for dt in (np.float32, np.float64):
            _check(op, seg, s, f, M.values(len(s), dt), mseg, ms, mf, name)


def test_forty_thousand_runs_against_five_thousand_masks():
    import cover_model as CM
    rng = np.random.default_rng(8)
    s, f = M.disjoint_segment(rng, 40000, 1000000)
    ms, mf = CM.random_segment(rng, 5000, 1000000, 300)
    seg, mseg = np.array([0, len(s)], np.int64), np.array([0, len(ms)], np.int64)
    assert len(s) == 40000
    for op in OPS:
        _check(op, seg, s, f, M.values(len(s), np.float32), mseg, ms, mf)
    so, fo = CM.random_segment(rng, 40000, 1000000, 150)         # a source that overlaps itself
    for op in ("overlaps", "noverlaps", "nearest"):
        _check(op, seg, so, fo, M.values(len(so), np.float64), mseg, ms, mf)


def test_capacity_exact_and_one_short():
    from wiggletools_amd import engine
    src, mask = SEAMS["segments"]
    seg, s, f = M.flat(src)
    mseg, ms, mf = M.flat(mask)
    v = np.ones(len(s), np.float32)
    for op in OPS:
        need = len(M.segmented(op, seg, s, f, v, mseg, ms, mf)[1])
        rc, n_out, got = engine._region_door(op, _rl(seg, s, f), _rl(mseg, ms, mf), capacity=need)
        assert (rc, n_out) == (OK, need) and len(got.start) == need, op
        assert engine._region_door(op, _rl(seg, s, f), _rl(mseg, ms, mf), capacity=need - 1)[:2] == (ERR_CAPACITY, need), op


def test_refusals():
    from wiggletools_amd import engine
    src, mask = SEAMS["segments"]
    seg, s, f = M.flat(src)
    mseg, ms, mf = M.flat(mask)
    door = lambda op, a, b, c, d: engine._region_door(op, _rl(seg, a, b), _rl(mseg, c, d))[0]      # noqa: E731
    assert door(4, s, f, ms, mf) == ERR_ARG and door(-1, s, f, ms, mf) == ERR_ARG
    s2 = s.copy(); s2[5], s2[6] = s[6], s[5]
    f3 = f.copy(); f3[9] = s[9]
    ms2 = ms.copy(); ms2[2], ms2[3] = max(ms[2], ms[3]) + 1, min(ms[2], ms[3])
    mf2 = np.maximum(mf, ms2 + 1)
    mf3 = mf.copy(); mf3[4] = ms[4]
    for op in OPS:
        assert door(op, s, f, ms, mf) == OK
        for args in ((s2, f, ms, mf), (s, f3, ms, mf), (s, f, ms2, mf2), (s, f, ms, mf3)):
            assert door(op, *args) == ERR_ARG, op
    f4 = f.copy(); f4[3] = s[4] + 1                  # runs 3 and 4 overlap: only a trim minds
    assert door("trim", s, f4, ms, mf) == ERR_ARG and door("overlaps", s, f4, ms, mf) == OK
    for name in ("n%d_overlapping" % (M.constants()[0] + 1),):
        a, b = SEAMS[name]
        assert engine._region_door("trim", _rl(*M.flat(a)), _rl(*M.flat(b)))[0] == ERR_ARG
    with pytest.raises(Exception):
        engine.region_runlists("trim", _rl(seg, s, f4), _rl(mseg, ms, mf))


def test_dropin_region_iterator(oracle, monkeypatch):
    """wtamd_RegionIterator in the product: pop(), blocks, seek, Multiplexer children under MeanReduction -- through the device
    door, then with WTAMD_NO_DEVICE_REGION=1 through the host sweep: the same lists."""
    from wiggletools_amd import _lib
    _lib.lib()
    D = region_dropin.DropIn(_lib.LIB_PATH)
    fixtures = region_dropin.load_fixtures()
    region_dropin.check_dropin(D, oracle, fixtures, np.random.default_rng(3))
    rng = np.random.default_rng(4)
    names = ["chr1", "chr2"]
    case = region_dropin.random_case(rng, names, 5000, 200000, False)
    seg, s, f, v, mseg, ms, mf = case

    def read(op):
        return D.read_blocks(D.region(op, D.reader(names, seg, s, f, v, overlapping=False), D.reader(names, mseg, ms, mf, np.ones(len(ms), np.float32))))
    dev = {op: read(op) for op in OPS}
    monkeypatch.setenv("WTAMD_NO_DEVICE_REGION", "1")
    for op in OPS:
        assert region_dropin.same_rows(dev[op], read(op)) and region_dropin.same_rows(dev[op], region_dropin.expected_rows(op, names, *case)), op
    region_dropin.check_dropin(D, oracle, fixtures, np.random.default_rng(3))
