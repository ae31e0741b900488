"""Coverage and union of overlapping intervals on the device (csrc/wt_cover.hip: wtamd_runs_coverage, wtamd_runs_union,
wtamd_CoverageIterator) against the NumPy model of tests/cover_model.py, which tests/test_cover_model.py pins to output
recorded from the compiled reference.  Every comparison is exact: coordinates, offsets, integer depths, value bits."""
import json
import os

import numpy as np
import pytest

import cover_model as M

SEAMS = M.seam_cases()
_flat = M.flat

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
OK, ERR_ARG, ERR_CAPACITY = 0, 1, 3


def _rl(seg, s, f, v=None):
    from wiggletools_amd.runlists import RunLists
    return RunLists(len(seg) - 1, 1, seg, s, f, np.ones(len(s), np.float32) if v is None else v)


def _check_coverage(seg, s, f, what=""):
    from wiggletools_amd import engine
    got = engine.coverage_runlists(_rl(seg, s, f))
    exp = M.segmented(M.coverage, seg, s, f)
    assert np.array_equal(got.seg_off, exp[0]), what
    assert np.array_equal(got.start, exp[1]) and np.array_equal(got.finish, exp[2]) and M.same_bits(got.value, exp[3]), what
    assert np.array_equal(got.defaults, np.zeros(got.n_tracks))


def _check_union(seg, s, f, v, what=""):
    from wiggletools_amd import engine
    got = engine.union_runlists(_rl(seg, s, f, v))
    exp = M.segmented(M.union, seg, s, f, v)
    assert np.array_equal(got.seg_off, exp[0]), what
    assert np.array_equal(got.start, exp[1]) and np.array_equal(got.finish, exp[2]) and M.same_bits(got.value, exp[3]), what


def _values(n, dt, seed=1):
    """Values whose bits must arrive unchanged: NaN (with a payload in f64), -0.0, denormal, the rest random."""
    v = np.random.default_rng(seed).standard_normal(n).astype(dt)
    special = [np.nan, -0.0, np.finfo(dt).tiny / 4]
    if dt == np.float64:
        special.append(np.array([0x7ff8000000000123], np.uint64).view(np.float64)[0])
    for k, x in enumerate(special):
        v[k::max(n // 3, len(special))] = x
    return v


def test_fixtures_through_both_doors():
    with open(os.path.join(HERE, "golden", "coverage_fixtures.json")) as fh:
        cases = json.load(fh)["cases"]
    # every recorded case is a few segments; all of them in one call (some 400 segments), and the first few one by one
    seg = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(c["seg_off"]) for c in cases]))]).astype(np.int64)
    s = np.concatenate([c["start"] for c in cases]).astype(np.int32)
    f = np.concatenate([c["finish"] for c in cases]).astype(np.int32)
    v = np.concatenate([c["value"] for c in cases])
    _check_coverage(seg, s, f)
    _check_union(seg, s, f, v.astype(np.float32))
    _check_union(seg, s, f, v)
    for c in cases[:6]:
        a = (np.array(c["seg_off"], np.int64), np.array(c["start"], np.int32), np.array(c["finish"], np.int32))
        _check_coverage(*a, what=c["name"])
        _check_union(*a, np.array(c["value"]), what=c["name"])
        # against the recording itself, without the reference's run of start == finish
        from wiggletools_amd import engine
        got = engine.coverage_runlists(_rl(*a))
        cov = c["coverage"]
        _, cs, cf, cv, stripped = M.strip_zero_length(cov["chrom"], cov["start"], cov["finish"], cov["value"])
        assert stripped <= 1 and np.array_equal(got.start, cs) and np.array_equal(got.finish, cf) and np.array_equal(got.value, cv)


@pytest.mark.parametrize("name", sorted(SEAMS))
def test_seams(name):
    seg, s, f = _flat(SEAMS[name])
    _check_coverage(seg, s, f, name)
    for dt in (np.float32, np.float64):
        _check_union(seg, s, f, _values(len(s), dt), name)


def test_many_intervals_and_a_long_span():
    rng = np.random.default_rng(8)
    s, f = M.random_segment(rng, 40000, 1000003, 150)
    seg = np.array([0, len(s)], np.int64)
    _check_coverage(seg, s, f)
    _check_union(seg, s, f, _values(len(s), np.float32))


def test_one_interval_over_twenty_thousand_short_ones():
    """A non-zero depth carried through every block of the scan, through stretches without a breakpoint; for the union one group
    that spans every block of the prefix maximum."""
    rng = np.random.default_rng(9)
    short = np.sort(rng.integers(2, 3000000, 20000))
    s = np.concatenate([[1], short]).astype(np.int32)
    f = np.concatenate([[3000100], short + rng.integers(1, 5, 20000)]).astype(np.int32)
    seg = np.array([0, len(s)], np.int64)
    _check_coverage(seg, s, f)
    _check_union(seg, s, f, _values(len(s), np.float64))
    assert len(M.union(s, f, np.ones(len(s)))[0]) == 1


def test_five_thousand_identical_intervals():
    s, f = np.full(5000, 123, np.int32), np.full(5000, 4567, np.int32)
    seg = np.array([0, 5000], np.int64)
    _check_coverage(seg, s, f)
    from wiggletools_amd import engine
    got = engine.coverage_runlists(_rl(seg, s, f))
    assert (got.start.tolist(), got.finish.tolist(), got.value.tolist()) == ([123], [4567], [5000.0])
    _check_union(seg, s, f, _values(5000, np.float32))


def test_small_scratch_budget_groups_segments_and_cuts_at_positions(monkeypatch):
    """1 MiB of bitmap and ranks = 5.6 Mbp a pass: the small segments go two at a time, the 3e7-bp one in six pieces -- with
    an interval across five of the cuts, a piece that holds no breakpoint under it, and a stretch of depth 0 across a cut."""
    monkeypatch.setenv("WTAMD_COVER_SCRATCH_MB", "1")
    rng = np.random.default_rng(10)
    pos = np.concatenate([rng.integers(2000, 5500000, 6000), rng.integers(12000000, 21000000, 6000), rng.integers(24000000, 29999000, 6000)])
    pos = np.sort(pos)
    s = np.concatenate([[1000], pos]).astype(np.int32)
    f = np.concatenate([[22000000], pos + rng.integers(1, 400, len(pos))]).astype(np.int32)
    o = np.argsort(s, kind="stable")
    big = (s[o], f[o])
    small = [M.random_segment(rng, 300, 2000000, 200) for _ in range(5)]
    empty = (np.zeros(0, np.int32), np.zeros(0, np.int32))
    seg, s, f = _flat(small[:2] + [empty, big, empty] + small[2:])
    _check_coverage(seg, s, f)


def test_capacity_exact_and_one_short():
    from wiggletools_amd import engine
    seg, s, f = _flat(SEAMS["segments"])
    need = len(M.segmented(M.coverage, seg, s, f)[1])
    rc, n_out, got = engine._overlap_door(_rl(seg, s, f), False, capacity=need)
    assert (rc, n_out) == (OK, need) and len(got.start) == need
    rc, n_out, got = engine._overlap_door(_rl(seg, s, f), False, capacity=need - 1)
    assert (rc, n_out) == (ERR_CAPACITY, need)
    needu = len(M.segmented(M.union, seg, s, f, np.ones(len(s)))[1])
    assert engine._overlap_door(_rl(seg, s, f), True, capacity=needu)[:2] == (OK, needu)
    assert engine._overlap_door(_rl(seg, s, f), True, capacity=needu - 1)[:2] == (ERR_CAPACITY, needu)


def test_unsorted_segment_is_refused():
    from wiggletools_amd import engine
    seg, s, f = _flat(SEAMS["segments"])
    s2 = s.copy()
    s2[5], s2[6] = max(s[5], s[6]) + 1, min(s[5], s[6])
    f2 = np.maximum(f, s2 + 1)
    for union in (False, True):
        assert engine._overlap_door(_rl(seg, s2, f2), union)[0] == ERR_ARG
    f3 = f.copy()
    f3[9] = s[9]
    for union in (False, True):
        assert engine._overlap_door(_rl(seg, s, f3), union)[0] == ERR_ARG
    with pytest.raises(Exception):
        engine.coverage_runlists(_rl(seg, s2, f2))


def test_dropin_coverage_iterator(oracle, monkeypatch):
    """wtamd_CoverageIterator over wtamd_OverlappingArrayReader in the product: pop(), blocks, seek, Multiplexer children under
    MeanReduction -- through the device door, then with WTAMD_NO_DEVICE_COVERAGE=1 through the host sweep: the same lists."""
    import cover_dropin
    from wiggletools_amd import _lib
    _lib.lib()
    D = cover_dropin.DropIn(_lib.LIB_PATH)
    cover_dropin.check_dropin(D, oracle, np.random.default_rng(3))
    rng = np.random.default_rng(4)
    names = ["chr1", "chr2"]
    (seg, s, f), = cover_dropin.tracks_case(rng, 1, 2, 5000, 200000, 300)
    dev = D.read_blocks(D.coverage(D.reader(names, seg, s, f, np.ones(len(s), np.float32))))
    monkeypatch.setenv("WTAMD_NO_DEVICE_COVERAGE", "1")
    host = D.read_blocks(D.coverage(D.reader(names, seg, s, f, np.ones(len(s), np.float32))))
    assert dev == host == cover_dropin.expected_rows(names, seg, s, f)
    cover_dropin.check_dropin(D, oracle, np.random.default_rng(3))
