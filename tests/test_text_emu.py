"""The passes of csrc/wt_text.h run through the CPU emulator (tests/text_emu.cpp: the product's own door over a launcher that
runs the workgroups forwards, backwards or shuffled) and the product's host sweep, on every case of text_model.cases(): byte
for byte the Python model's text, which tests/golden/make_text_golden.py holds to the compiled reference's and whose recorded
form (tests/golden/text_fixtures.json) is checked here as well."""
import numpy as np
import pytest

import text_model as M

CASES = M.cases()


def _door(order, seed=7):
    def door(L, flags, state=None, capacity=None, offset=0, dtype=np.float64, names=None, seg=None, n_seg=None):
        return M.emu_call(L, flags, state, capacity, offset, order, seed, dtype, names, seg, n_seg)
    return door


DOORS = {"forwards": _door(0), "backwards": _door(1), "shuffled": _door(2), "host sweep": M.host_call}


@pytest.fixture(scope="module")
def reference_texts():
    """The model's text of every case in both modes, held to what the compiled reference printed."""
    out = {}
    every = M.reference_cases()
    for c in M.fixtures():
        L = every[c["case"]]
        out[c["name"]] = M.text(L, c["flags"])[0]
        M.check_against_fixture(c, L, c["flags"], out[c["name"]])
    assert len(out) == 2 * len(every)
    return out


@pytest.mark.parametrize("how", sorted(DOORS))
def test_every_case_in_both_modes_is_the_reference_text(how, reference_texts):
    for name, L in CASES.items():
        for flags in (0, M.BEDGRAPH):
            got = M.check_case(DOORS[how], L, flags, (name, flags, how))
            assert got == reference_texts["%s/%d" % (name, flags)]


@pytest.mark.parametrize("how", sorted(DOORS))
def test_f32_input_is_the_widened_values(how):
    for name in ("values_f32", "random_257", "transitions_gaps"):
        L = CASES[name].as_f32()
        for flags in (0, M.BEDGRAPH):
            a = M.check_case(DOORS[how], L, flags, (name, how), dtype=np.float32)
            assert a == M.check_case(DOORS[how], L, flags, (name, how), dtype=np.float64)


@pytest.mark.parametrize("how", sorted(DOORS))
def test_cut_lists_chain_through_the_state(how):
    for name in ("random_20001", "straddle_10000", "points_across_10000", "chrom_change", "random_257"):
        for flags in (0, M.BEDGRAPH):
            M.check_chained(DOORS[how], CASES[name], flags, (name, flags, how))


@pytest.mark.parametrize("how", sorted(DOORS))
def test_any_alignment_and_the_exact_capacity(how):
    for name in ("random_257", "random_10001", "names"):
        M.check_alignment_and_capacity(DOORS[how], CASES[name], 0, (name, how))


@pytest.mark.parametrize("how", ["forwards", "shuffled"])
def test_refusals_write_nothing(how):
    M.check_refusals(DOORS[how])


@pytest.mark.parametrize("how", sorted(DOORS))
def test_run_counts_and_offsets_the_door_refuses(how):
    M.check_count_refusals(DOORS[how])


def test_the_host_sweep_prints_wide_values():
    """snprintf on the host: the text of a batch the device refuses; its other refusals are the door's."""
    for W, n_wide in M.wide_lists():
        for flags in (0, M.BEDGRAPH):
            want = M.text(W, flags)[0]
            rc, buf, nb, nw, _ = M.host_call(W, flags, capacity=len(want))
            assert (rc, nb, nw) == (0, len(want), n_wide) and M.payload(buf, 0, nb) == want
    for name, L, flags, state in M.refusals():
        rc, buf, nb, nw, st = M.host_call(L, flags, state=state if state is not None else M.fresh_state(), capacity=1 << 20)
        assert rc == M.ERR_ARG and (buf == M.CANARY).all(), name


def test_an_empty_call_leaves_the_state_alone():
    L = CASES["random_255"].part(0, 0)
    st = {"in_block": 17, "point_by_point": 1, "last_finish": 99, "continues": 0}
    for how in sorted(DOORS):
        rc, buf, nb, nw, st2 = DOORS[how](L, 0, state=st, capacity=0)
        assert (rc, nb, nw, st2) == (0, 0, 0, st) and (buf == M.CANARY).all(), how


def test_one_workgroup_per_block_of_the_reference():
    import ctypes as C
    L = CASES["random_20001"]
    n = C.c_int64()
    want = M.text(L, 0)[0]
    buf = np.zeros(len(want), np.uint8)
    arr = (C.c_char_p * len(L.names))(*L.names)
    nb, nw = C.c_int64(), C.c_int64()
    p = lambda x: C.c_void_p(x.ctypes.data)      # noqa: E731
    rc = M.emu_lib().text_emu_door(C.c_int(0), C.c_uint64(1), C.c_int64(len(L.names)), p(L.seg), arr, p(L.s), p(L.f), p(L.v), C.c_int(1), C.c_uint32(0),
                                   None, p(buf), C.c_int64(len(want)), C.byref(nb), C.byref(nw), C.byref(n))
    assert rc == 0 and n.value == 3 and buf.tobytes() == want      # measure, scan, emit
    assert M.constants()["ENTRIES"] == M.BLOCK


def test_the_integer_lf_on_the_special_values():
    for v in M.special_values():
        assert M.fmt_c(v) == M.fmt(v), (v, M.fmt_c(v), M.fmt(v))
    assert M.fmt_c(2.0 ** 64) is None and M.fmt_c(-1.7976931348623157e308) is None
    assert [M.fmt_c(x) for x in (0.0078125, 0.0234375, 9.9999995, 0.9999995, 1.0000005)] == ["0.007812", "0.023438", "9.999999", "1.000000", "1.000001"]
