"""Coverage of intervals in ANY order inside a segment (wtamd_runs_coverage_flags, WTAMD_COVER_ANY_ORDER), on the CPU: the door
and the passes of csrc/wt_cover.h run workgroup by workgroup, forwards, backwards and shuffled (tests/cover_any_emu.cpp).  The
result must be, byte for byte, the coverage of the same intervals sorted by start -- by the model of tests/cover_model.py and
by the door without the flag.  The same cases run on the device in tests/test_cover_any_order_gpu.py."""
import numpy as np
import pytest

import cover_any_cases as A
import cover_model as M

CASES = A.cases()
OK, ERR_ARG, ERR_CAPACITY = 0, 1, 3


def _same(got, exp):
    rc, n_out, oseg, os_, of, ov = got[:6]
    return (rc == OK and n_out == len(exp[1]) and np.array_equal(oseg, exp[0]) and np.array_equal(os_, exp[1]) and
            np.array_equal(of, exp[2]) and M.same_bits(ov, exp[3]))


def _check(segs, budget=256 << 20, what=""):
    """Any order == model == the door with flags 0 over the sorted list; returns the launches of the any-order call."""
    exp = A.expected(segs)
    seg, s, f = M.flat(segs)
    launches = None
    for order in (0, 1, 2):
        got = A.emu_coverage(seg, s, f, A.ANY_ORDER, order=order, seed=13, budget=budget)
        assert _same(got, exp), (what, order)
        launches = got[6]
    sseg, ss, sf = M.flat(A.sorted_by_start(segs))
    plain = A.emu_coverage(sseg, ss, sf, 0, budget=budget)
    assert _same(plain, exp), what
    assert plain[6] == launches, what                       # the same passes: nothing is sorted on the way
    return launches


@pytest.mark.parametrize("name", sorted(CASES))
def test_any_order_equals_the_sorted_input(name):
    assert A.is_unsorted(CASES[name]) or name == "identical"
    _check(CASES[name], what=name)


def test_reads_of_sam_text_give_what_the_compiled_reference_pops():
    """The components of the reads of SAM text in file order (the reference's test/sam.sam, a hand-made text with every CIGAR
    op) against the pops recorded from the compiled reference's SamReader (tests/golden/make_sam_cover_golden.py)."""
    for name, segs, pops in A.sam_fixtures():
        assert A.is_unsorted(segs), name
        seg, s, f = M.flat(segs)
        for order in (0, 1, 2):
            assert _same(A.emu_coverage(seg, s, f, A.ANY_ORDER, order=order, seed=14), pops), (name, order)
        assert _same(A.emu_coverage(seg, s, f, A.ANY_ORDER, budget=12 * 7), pops), name
        assert A.emu_coverage(seg, s, f, 0)[0] == ERR_ARG, name


def test_flags_zero_still_refuses_what_the_flag_takes():
    for name in sorted(CASES):
        if not A.is_unsorted(CASES[name]):
            continue
        seg, s, f = M.flat(CASES[name])
        assert A.emu_coverage(seg, s, f, 0)[0] == ERR_ARG, name
        assert M.emu_coverage(seg, s, f)[0] == ERR_ARG, name            # the entry without flags (tests/cover_emu.cpp)


def test_sorted_input_gives_the_same_with_and_without_the_flag():
    for name in ("segments", "segments50", "carry", "touching", "n257", "span131072b"):
        seg, s, f = M.flat(M.seam_cases()[name])
        a = A.emu_coverage(seg, s, f, A.ANY_ORDER)
        b = M.emu_coverage(seg, s, f)
        assert a[0] == b[0] == OK and a[1] == b[1], name
        for k in (2, 3, 4):
            assert np.array_equal(a[k], b[k]), name
        assert M.same_bits(a[5], b[5]), name


def test_cut_at_positions_and_grouped_under_a_small_budget():
    # 12 bytes per 64 positions: 60 bytes = 320 positions a pass
    plain = _check(CASES["spliced"])
    cut = _check(CASES["spliced"], budget=60, what="spliced")
    assert cut > 20 * plain                                  # (60 000 bp in pieces of 320)
    for name in ("min_last", "min_middle", "issue_trap", "two", "break_at_block_seam", "min_in_second_block", "identical",
                 "breaks_across_segment_boundaries", "boundary_at_block_seam"):
        _check(CASES[name], budget=12 * 7, what=name)        # 448 positions
    _check(CASES["long_one_last"], budget=12 * 100, what="long_one_last")        # 6400 positions: 32 pieces, each entered with a carry
    one = _check(CASES["segments50"])
    grouped = _check(CASES["segments50"], budget=12 * 100, what="segments50")
    assert grouped > 3 * one


def test_capacity_and_validation():
    segs = CASES["breaks_across_segment_boundaries"]
    seg, s, f = M.flat(segs)
    need = len(A.expected(segs)[1])
    rc, n_out, *_ = A.emu_coverage(seg, s, f, A.ANY_ORDER, capacity=need)
    assert (rc, n_out) == (OK, need)
    rc, n_out, *_ = A.emu_coverage(seg, s, f, A.ANY_ORDER, capacity=need - 1)
    assert (rc, n_out) == (ERR_CAPACITY, need)
    # start >= finish is refused in any order, and so is a flag nobody defined
    for bad in (s[9], s[9] - 1):
        f3 = f.copy()
        f3[9] = bad
        assert A.emu_coverage(seg, s, f3, A.ANY_ORDER)[0] == ERR_ARG
    assert A.emu_coverage(seg, s, f, 2)[0] == ERR_ARG and A.emu_coverage(seg, s, f, A.ANY_ORDER | 4)[0] == ERR_ARG
    # nothing to do
    rc, n_out, oseg, *_ = A.emu_coverage(np.zeros(4, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32), A.ANY_ORDER)
    assert (rc, n_out, oseg.tolist()) == (OK, 0, [0, 0, 0, 0])
