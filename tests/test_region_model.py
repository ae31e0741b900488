"""The region operators (overlaps, noverlaps, trim, nearest) on the CPU: the NumPy model (tests/region_model.py) against output
recorded from the compiled reference (tests/golden/region_fixtures.json), the passes of csrc/wt_region.h run workgroup by
workgroup in any order (tests/region_emu.cpp) against the model, and wtamd_RegionIterator in the emulated drop-in library (host
sweep: that library holds no HIP unit).  The same cases run on the device in tests/test_region_gpu.py.  Every comparison is
exact: coordinates, offsets and value bits."""
import numpy as np
import pytest

import region_dropin
import region_model as M

OK, ERR_ARG, ERR_CAPACITY = 0, 1, 3
OPS = sorted(M.OPS, key=M.OPS.get)


@pytest.fixture(scope="module")
def fixtures():
    return region_dropin.load_fixtures()


def test_model_equals_the_compiled_reference(fixtures):
    assert len(fixtures) >= 150
    seen = {op: 0 for op in OPS}
    for c in fixtures:
        seg, s, f, v, mseg, ms, mf = region_dropin.case_arrays(c)
        for op in OPS:
            if op not in c:
                assert op == "trim" and c["source"]["overlaps"]
                continue
            rec = c[op]
            oseg, es, ef, ev = M.segmented(op, seg, s, f, v, mseg, ms, mf)
            assert np.array_equal(rec["start"], es) and np.array_equal(rec["finish"], ef), (c["name"], op)
            assert M.same_bits(region_dropin.recorded_values(rec), ev), (c["name"], op)
            assert np.array_equal(np.searchsorted(rec["chrom"], np.arange(len(seg))), oseg), (c["name"], op)
            seen[op] += 1
    assert min(seen.values()) >= 90, seen


def test_trim_of_an_overlapping_source_is_the_reference_protocol(fixtures):
    """What the reference's trim does with a source that overlaps itself depends on its pop order: the model of that protocol
    equals the recording, the rule of the device door does not always -- which is why the door refuses such a source."""
    n = differ = 0
    for c in fixtures:
        if "trim_overlapping_source" not in c:
            continue
        seg, s, f, v, mseg, ms, mf = region_dropin.case_arrays(c)
        rec = c["trim_overlapping_source"]
        oseg, es, ef, ev = M.segmented("trim", seg, s, f, v, mseg, ms, mf, fn=M.trim_protocol)
        assert np.array_equal(rec["start"], es) and np.array_equal(rec["finish"], ef) and M.same_bits(rec["value"], ev), c["name"]
        rule = M.segmented("trim", seg, s, f, v, mseg, ms, mf)
        differ += not (np.array_equal(rule[1], es) and np.array_equal(rule[2], ef))
        n += 1
        if M.overlaps_itself(seg, s, f):
            assert M.emu_region("trim", seg, s, f, v, mseg, ms, mf)[0] == ERR_ARG, c["name"]
    assert n >= 40 and differ >= 5, (n, differ)


def _check_emu(op, seg, s, f, v, mseg, ms, mf, what=""):
    exp = M.segmented(op, seg, s, f, v, mseg, ms, mf)
    for o in (0, 1, 2):
        rc, n_out, oseg, os_, of, ov, _ = M.emu_region(op, seg, s, f, v, mseg, ms, mf, order=o, seed=13)
        assert rc == OK and n_out == len(exp[1]), (what, op)
        assert np.array_equal(oseg, exp[0]) and np.array_equal(os_, exp[1]) and np.array_equal(of, exp[2]) and M.same_bits(ov, exp[3]), (what, op)


def test_emulated_passes_on_the_fixtures_in_any_block_order(fixtures):
    for c in fixtures:
        seg, s, f, v, mseg, ms, mf = region_dropin.case_arrays(c)
        for op in OPS:
            if op in c:
                _check_emu(op, seg, s, f, v.astype(np.float32), mseg, ms, mf, what=c["name"])
    # all of them in one call: some 300 segments
    for op in OPS:
        _check_emu(op, *region_dropin.all_in_one(fixtures, op), what="all")


SEAMS = M.seam_cases()


@pytest.mark.parametrize("name", sorted(SEAMS))
def test_emulated_passes_at_the_seams(name):
    src, mask = SEAMS[name]
    seg, s, f = M.flat(src)
    mseg, ms, mf = M.flat(mask)
    for op in OPS:
        if op == "trim" and M.overlaps_itself(seg, s, f):
            assert M.emu_region(op, seg, s, f, M.values(len(s), np.float32), mseg, ms, mf)[0] == ERR_ARG
            continue
        for dt in (np.float32, np.float64):
            _check_emu(op, seg, s, f, M.values(len(s), dt), mseg, ms, mf, what=name)


def test_seam_cases_are_what_they_claim():
    T, W = M.constants()
    src, mask = SEAMS["wide_trim"]
    seg, s, f = M.flat(src)
    gs, gf, _ = M.CM.union(mask[0][0], mask[0][1], np.zeros(len(mask[0][0])))
    met = np.searchsorted(gs, f[T - 1], side="left") - np.searchsorted(gf, s[T - 1], side="right")
    assert met == 2 * T + 3 and len(s) > T
    for w in (W, W + 1):
        src, mask = SEAMS["window%d" % w]
        assert len(src[0][0]) <= T and len(mask[0][0]) == w
        assert len(M.region("trim", src[0][0], src[0][1], np.zeros(len(src[0][0])), *mask[0])[0]) >= w
    src, mask = SEAMS["segments"]
    assert sum(len(x[0]) for x in src) < T
    kinds = {(len(a[0]) > 0, len(b[0]) > 0) for a, b in zip(src, mask)}
    assert kinds == {(True, True), (True, False), (False, True), (False, False)}
    # strictness and the nearest quirks, spelled out
    (s, f), = SEAMS["strict"][0]
    (ms, mf), = SEAMS["strict"][1]
    assert M.region("overlaps", s, f, np.arange(4.0), ms, mf)[2].tolist() == [3.0]
    assert M.region("noverlaps", s, f, np.arange(4.0), ms, mf)[2].tolist() == [0.0, 1.0, 2.0]
    assert [tuple(x.tolist()) for x in M.region("trim", s, f, np.arange(4.0), ms, mf)] == [(40,), (41,), (3.0,)]
    (s, f), = SEAMS["nearest"][0]
    (ms, mf), = SEAMS["nearest"][1]
    assert M.region("nearest", s, f, np.zeros(5), ms, mf)[2].tolist() == [6.0, 0.0, 3.0, 0.0, 41.0]
    assert np.isnan(M.region("nearest", [3], [5], [0.0], [], [])[2]).all()


def test_emulated_capacity_and_refusals():
    src, mask = SEAMS["segments"]
    seg, s, f = M.flat(src)
    mseg, ms, mf = M.flat(mask)
    v = np.ones(len(s), np.float32)
    for op in OPS:
        need = len(M.segmented(op, seg, s, f, v, mseg, ms, mf)[1])
        assert M.emu_region(op, seg, s, f, v, mseg, ms, mf, capacity=need)[:2] == (OK, need)
        rc, n_out, *_, untouched = M.emu_region(op, seg, s, f, v, mseg, ms, mf, capacity=need - 1)
        assert (rc, n_out, untouched) == (ERR_CAPACITY, need, True), op
    # unknown operator; unsorted and start >= finish on either side; a trim source that overlaps itself
    assert M.emu_region(4, seg, s, f, v, mseg, ms, mf)[0] == ERR_ARG and M.emu_region(-1, seg, s, f, v, mseg, ms, mf)[0] == ERR_ARG
    s2 = s.copy(); s2[5], s2[6] = s[6], s[5]
    f3 = f.copy(); f3[9] = s[9]
    ms2 = ms.copy(); ms2[2], ms2[3] = max(ms[2], ms[3]) + 1, min(ms[2], ms[3])
    mf2 = np.maximum(mf, ms2 + 1)
    mf3 = mf.copy(); mf3[4] = ms[4]
    for op in OPS:
        for args in ((s2, f, ms, mf), (s, f3, ms, mf), (s, f, ms2, mf2), (s, f, ms, mf3)):
            rc, _, _, _, _, _, untouched = M.emu_region(op, seg, args[0], args[1], v, mseg, args[2], args[3])
            assert (rc, untouched) == (ERR_ARG, True), op
    f4 = f.copy(); f4[3] = s[4] + 1
    assert s[4] > s[3] and M.emu_region("trim", seg, s, f4, v, mseg, ms, mf)[0] == ERR_ARG
    assert M.emu_region("overlaps", seg, s, f4, v, mseg, ms, mf)[0] == OK
    # a start below the one in front of it at a segment boundary is fine
    assert s[seg[2]] < s[seg[2] - 1]


def test_dropin_region_iterator_on_the_host(oracle, fixtures):
    """wtamd_RegionIterator in the emulated drop-in library (no HIP unit: the weak reference to the device door is null and
    the iterator sweeps on the host)."""
    from emu import build as emu_build
    D = region_dropin.DropIn(emu_build.build_dropin())
    region_dropin.check_dropin(D, oracle, fixtures, np.random.default_rng(3))
