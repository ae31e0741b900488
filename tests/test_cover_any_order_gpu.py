"""Coverage of intervals in ANY order inside a segment on the device (csrc/wt_cover.hip: wtamd_runs_coverage_flags with
WTAMD_COVER_ANY_ORDER, wtamd_runs_coverage_host_flags): the cases of tests/test_cover_any_order_emu.py, every comparison
exact -- coordinates, offsets, integer depths -- against the model over the same intervals sorted by start and against the
door without the flag over that sorted list."""
import ctypes as C

import numpy as np
import pytest

import cover_any_cases as A
import cover_model as M

pytestmark = pytest.mark.gpu

CASES = A.cases()
OK, ERR_ARG, ERR_CAPACITY = 0, 1, 3


def _rl(segs):
    from wiggletools_amd.runlists import RunLists
    seg, s, f = M.flat(segs)
    return RunLists(len(seg) - 1, 1, seg, s, f, np.ones(len(s), np.float32))


def _same(got, exp):
    return (np.array_equal(got.seg_off, exp[0]) and np.array_equal(got.start, exp[1]) and np.array_equal(got.finish, exp[2]) and
            M.same_bits(got.value, exp[3]))


def _check(segs, what=""):
    from wiggletools_amd import engine
    exp = A.expected(segs)
    assert _same(engine.coverage_runlists(_rl(segs), any_order=True), exp), what
    assert _same(engine.coverage_runlists(_rl(A.sorted_by_start(segs))), exp), what


@pytest.mark.parametrize("name", sorted(CASES))
def test_any_order_equals_the_sorted_input(name):
    _check(CASES[name], name)


def test_reads_of_sam_text_give_what_the_compiled_reference_pops():
    """The components of the reads of SAM text in file order against the pops recorded from the compiled reference's SamReader
    (tests/golden/sam_cover_fixtures.json)."""
    from wiggletools_amd import engine
    for name, segs, pops in A.sam_fixtures():
        assert _same(engine.coverage_runlists(_rl(segs), any_order=True), pops), name
        assert engine._overlap_door(_rl(segs), False)[0] == ERR_ARG, name


def test_flags_zero_still_refuses_what_the_flag_takes():
    from wiggletools_amd import engine
    for name in ("min_last", "issue_trap", "break_at_block_seam", "breaks_across_segment_boundaries", "spliced"):
        assert A.is_unsorted(CASES[name])
        assert engine._overlap_door(_rl(CASES[name]), False)[0] == ERR_ARG, name
        assert engine._overlap_door(_rl(CASES[name]), False, flags=0)[0] == ERR_ARG, name
    with pytest.raises(Exception):
        engine.coverage_runlists(_rl(CASES["issue_trap"]))


def test_sorted_input_gives_the_same_with_and_without_the_flag():
    from wiggletools_amd import engine
    for name in ("segments", "carry", "span131072b"):
        segs = M.seam_cases()[name]
        a, b = engine.coverage_runlists(_rl(segs), any_order=True), engine.coverage_runlists(_rl(segs))
        assert _same(a, (b.seg_off, b.start, b.finish, b.value)), name


def test_small_scratch_budget_groups_segments_and_cuts_at_positions(monkeypatch):
    """1 MiB of bitmap and ranks = 5.6 Mbp a pass: the small segments go two at a time, the 1.3e7-bp one in three pieces."""
    monkeypatch.setenv("WTAMD_COVER_SCRATCH_MB", "1")
    segs = A.pieces_case()
    big = max(segs, key=lambda x: len(x[0]))
    assert A.is_unsorted([big]) and int(big[1].max()) - int(big[0].min()) > 2 * 5592384
    _check(segs, "pieces")
    _check(CASES["long_one_last"], "long_one_last")


def test_capacity_and_validation():
    from wiggletools_amd import engine
    segs = CASES["breaks_across_segment_boundaries"]
    need = len(A.expected(segs)[1])
    rc, n_out, got = engine._overlap_door(_rl(segs), False, capacity=need, flags=A.ANY_ORDER)
    assert (rc, n_out) == (OK, need) and len(got.start) == need
    assert engine._overlap_door(_rl(segs), False, capacity=need - 1, flags=A.ANY_ORDER)[:2] == (ERR_CAPACITY, need)
    seg, s, f = M.flat(segs)
    f3 = f.copy()
    f3[9] = s[9]
    assert engine._overlap_door(_rl([(s, f3)]), False, flags=A.ANY_ORDER)[0] == ERR_ARG
    assert engine._overlap_door(_rl(segs), False, flags=2)[0] == ERR_ARG
    assert engine._overlap_door(_rl(segs), False, flags=A.ANY_ORDER | 4)[0] == ERR_ARG


def test_host_twin():
    """One segment in host arrays: any order with the flag, refused without it, the entry without flags as before."""
    from wiggletools_amd import _lib
    L = _lib.lib()
    (s, f), = CASES["min_in_second_block"]
    exp = A.expected([(s, f)])
    cap = 2 * len(s)

    def call(fn, s, f, *flags):
        os_, of, ov, n = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.float64), C.c_int64()
        rc = fn(len(s), s.ctypes.data, f.ctypes.data, cap, os_.ctypes.data, of.ctypes.data, ov.ctypes.data, C.byref(n), *flags)
        return rc, os_[:n.value], of[:n.value], ov[:n.value]

    rc, os_, of, ov = call(L.wtamd_runs_coverage_host_flags, s, f, A.ANY_ORDER)
    assert rc == OK and np.array_equal(os_, exp[1]) and np.array_equal(of, exp[2]) and M.same_bits(ov, exp[3])
    assert call(L.wtamd_runs_coverage_host_flags, s, f, 0)[0] == ERR_ARG
    assert call(L.wtamd_runs_coverage_host, s, f)[0] == ERR_ARG
    (ss, sf), = A.sorted_by_start([(s, f)])
    rc, os_, of, ov = call(L.wtamd_runs_coverage_host, ss, sf)
    assert rc == OK and np.array_equal(os_, exp[1]) and np.array_equal(of, exp[2]) and M.same_bits(ov, exp[3])
