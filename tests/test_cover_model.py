"""Coverage and union of overlapping intervals, on the CPU: the NumPy model (tests/cover_model.py) against output recorded from
the compiled reference (tests/golden/coverage_fixtures.json), the passes of csrc/wt_cover.h run workgroup by workgroup in any
order (tests/cover_emu.cpp) against the model, and the drop-in constructors in the emulated drop-in library (host sweep: that
library holds no HIP unit).  The same cases run on the device in tests/test_cover_gpu.py."""
import json
import os

import numpy as np
import pytest

import cover_model as M

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fixtures():
    with open(os.path.join(HERE, "golden", "coverage_fixtures.json")) as fh:
        return json.load(fh)["cases"]


def _arrays(c):
    return (np.array(c["seg_off"], np.int64), np.array(c["start"], np.int32), np.array(c["finish"], np.int32), np.array(c["value"], np.float64))


def test_model_equals_the_compiled_reference(fixtures):
    assert len(fixtures) >= 200
    for c in fixtures:
        seg, s, f, v = _arrays(c)
        cov = c["coverage"]
        ch, cs, cf, cv, stripped = M.strip_zero_length(cov["chrom"], cov["start"], cov["finish"], cov["value"])
        assert stripped <= 1, c["name"]             # the reference's one run of start == finish per stream (unaryOps.c:333-334)
        oseg, es, ef, ev = M.segmented(M.coverage, seg, s, f)
        assert np.array_equal(cs, es) and np.array_equal(cf, ef) and np.array_equal(cv, ev), c["name"]
        assert np.array_equal(np.searchsorted(ch, np.arange(len(seg))), oseg), c["name"]
        u = c["union"]
        useg, us, uf, uv = M.segmented(M.union, seg, s, f, v)
        assert np.array_equal(u["start"], us) and np.array_equal(u["finish"], uf) and M.same_bits(u["value"], uv), c["name"]
        assert np.array_equal(np.searchsorted(u["chrom"], np.arange(len(seg))), useg), c["name"]


def test_overlapping_bed_depth_track(fixtures):
    c = fixtures[0]
    assert c["name"] == "overlapping.bed"
    seg, s, f, _ = _arrays(c)
    oseg, es, ef, ev = M.segmented(M.coverage, seg, s, f)
    assert oseg.tolist() == [0, 3, 4]
    assert list(zip(es.tolist(), ef.tolist(), ev.tolist())) == [(2, 3, 1.0), (3, 6, 2.0), (6, 8, 1.0), (1, 4, 1.0)]


SEAMS = M.seam_cases()
_flat = M.flat


def _check_emu_coverage(seg, s, f, budget=256 << 20, what=""):
    exp = M.segmented(M.coverage, seg, s, f)
    results = [M.emu_coverage(seg, s, f, order=o, seed=11, budget=budget) for o in (0, 1, 2)]
    for rc, n_out, oseg, os_, of, ov, _ in results:
        assert rc == 0 and n_out == len(exp[1]), what
        assert np.array_equal(oseg, exp[0]) and np.array_equal(os_, exp[1]) and np.array_equal(of, exp[2]) and M.same_bits(ov, exp[3]), what
    return results[0][6]


def _check_emu_union(seg, s, f, v, what=""):
    exp = M.segmented(M.union, seg, s, f, v)
    for o in (0, 1, 2):
        rc, n_out, oseg, os_, of, ov = M.emu_union(seg, s, f, v, order=o, seed=12)
        assert rc == 0 and n_out == len(exp[1]), what
        assert np.array_equal(oseg, exp[0]) and np.array_equal(os_, exp[1]) and np.array_equal(of, exp[2]) and M.same_bits(ov, exp[3]), what


def test_emulated_passes_on_the_fixtures_in_any_block_order(fixtures):
    for c in fixtures[::4]:
        seg, s, f, v = _arrays(c)
        _check_emu_coverage(seg, s, f, what=c["name"])
        _check_emu_union(seg, s, f, v.astype(np.float32), what=c["name"])


@pytest.mark.parametrize("name", sorted(SEAMS))
def test_emulated_passes_at_the_seams(name):
    seg, s, f = _flat(SEAMS[name])
    _check_emu_coverage(seg, s, f, what=name)
    rng = np.random.default_rng(1)
    for dt in (np.float32, np.float64):
        v = rng.standard_normal(len(s)).astype(dt)
        if len(v) > 3:
            v[0], v[1], v[2] = np.nan, -0.0, np.array([0x7ff8000000000123], np.uint64).view(np.float64)[0] if dt == np.float64 else np.nan
        _check_emu_union(seg, s, f, v, what=name)


def test_emulated_scratch_budget_groups_segments_and_cuts_at_positions():
    seg, s, f = _flat(SEAMS["segments"])
    plain = _check_emu_coverage(seg, s, f)
    # 12 bytes per 64 positions: 60 bytes = 5 words = 320 positions a pass -- the 70 000-bp segment goes in 219 pieces
    cut = _check_emu_coverage(seg, s, f, budget=60)
    assert cut > 20 * plain
    seg, s, f = _flat(SEAMS["segments50"])
    one = _check_emu_coverage(seg, s, f)
    grouped = _check_emu_coverage(seg, s, f, budget=12 * 100)          # 6400 positions: a few segments per pass
    assert grouped > 3 * one
    for name in ("carry", "identical", "touching", "span131072a", "span131072b"):
        seg, s, f = _flat(SEAMS[name])
        _check_emu_coverage(seg, s, f, budget=12 * 7, what=name)


def test_emulated_capacity_and_validation():
    seg, s, f = _flat(SEAMS["segments"])
    exp = M.segmented(M.coverage, seg, s, f)
    need = len(exp[1])
    rc, n_out, *_ = M.emu_coverage(seg, s, f, capacity=need)
    assert rc == 0 and n_out == need
    rc, n_out, *_ = M.emu_coverage(seg, s, f, capacity=need - 1)
    assert rc == 3 and n_out == need
    v = np.ones(len(s), np.float32)
    needu = len(M.segmented(M.union, seg, s, f, v)[1])
    assert M.emu_union(seg, s, f, v, capacity=needu)[:2] == (0, needu)
    assert M.emu_union(seg, s, f, v, capacity=needu - 1)[:2] == (3, needu)
    # unsorted inside a segment, and start >= finish: refused; a start that falls at a segment boundary is fine
    s2 = s.copy(); s2[5], s2[6] = max(s[5], s[6]) + 1, min(s[5], s[6])
    f2 = np.maximum(f, s2 + 1)
    assert M.emu_coverage(seg, s2, f2)[0] == 1 and M.emu_union(seg, s2, f2, v)[0] == 1
    f3 = f.copy(); f3[9] = s[9]
    assert M.emu_coverage(seg, s, f3)[0] == 1 and M.emu_union(seg, s, f3, v)[0] == 1


def test_dropin_coverage_iterator_on_the_host(oracle):
    """wtamd_CoverageIterator over wtamd_OverlappingArrayReader in the emulated drop-in library (no HIP unit: the weak
    reference to the device door is null and the iterator sweeps on the host)."""
    from emu import build as emu_build
    import cover_dropin
    D = cover_dropin.DropIn(emu_build.build_dropin())
    cover_dropin.check_dropin(D, oracle, np.random.default_rng(3))
