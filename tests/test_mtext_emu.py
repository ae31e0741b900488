"""The passes of csrc/wt_mtext.h run through the CPU emulator (tests/mtext_emu.cpp: the product's own door over a launcher that
runs the workgroups of every pass forwards, backwards or shuffled) and the product's host sweep wtm_host, on every case of
mtext_model.cases(): byte for byte the Python model's text."""
import ctypes as C

import numpy as np
import pytest

import mtext_model as M

CASES = M.cases()


def _door(order, seed=7):
    def door(T, **kw):
        return M.emu_call(T, order=order, seed=seed, **kw)
    return door


def _host(T, **kw):
    return M.host_call(T, **kw)


DOORS = {"forwards": _door(0), "backwards": _door(1), "shuffled": _door(2), "host sweep": _host}


@pytest.mark.parametrize("how", sorted(DOORS))
def test_every_case_in_its_modes_is_the_model_text(how):
    for name, T in CASES.items():
        for flags in M.flags_of(T):
            M.check_case(DOORS[how], name, flags)


@pytest.mark.parametrize("how", sorted(DOORS))
def test_cut_tiles_chain_through_the_state(how):
    for name in ("w3_n20001", "straddle_10000_w2", "points_across_10000_w2", "chrom_change_w2", "w65_n257", "paste_w1_n10001"):
        for flags in M.flags_of(CASES[name]):
            M.check_chained(DOORS[how], name, flags)


@pytest.mark.parametrize("how", sorted(DOORS))
def test_any_alignment_and_the_exact_capacity(how):
    for name in ("w3_n257", "w2048_n40", "paste_w3"):
        M.check_alignment_and_capacity(DOORS[how], name, 0)


@pytest.mark.parametrize("how", ["forwards", "shuffled"])
def test_refusals_and_wide_cells_write_nothing(how):
    M.check_refusals(DOORS[how])


def test_the_host_sweep_prints_wide_cells_and_refuses_the_rest():
    for W, n_wide in M.wide_tiles():
        for flags in (0, M.BEDGRAPH):
            expect = M.text(W, flags)[0]
            rc, buf, nb, nw, _ = M.host_call(W, flags=flags, capacity=len(expect))
            assert (rc, nb, nw) == (0, len(expect), n_wide) and M.payload(buf, 0, nb) == expect
    for name, T, kw in M.refusals():
        kw = dict(dict(flags=0, state=M.fresh_state()), **kw)
        rc, buf, nb, nw, st = M.host_call(T, capacity=1 << 20, **kw)
        assert rc == M.ERR_ARG and (buf == M.CANARY).all() and st == kw["state"], name


def test_an_empty_call_leaves_the_state_alone():
    T = CASES["w3_n257"].part(0, 0)
    st = {"in_block": 17, "point_by_point": 1, "last_finish": 99, "continues": 0}
    for how in sorted(DOORS):
        rc, buf, nb, nw, st2 = DOORS[how](T, flags=0, state=st, capacity=0)
        assert (rc, nb, nw, st2) == (0, 0, 0, st) and (buf == M.CANARY).all(), how


def test_a_second_call_gives_the_same_bytes():
    for name in ("w64_n257", "paste_w3"):
        a = M.emu_call(CASES[name], order=2, seed=3, flags=0)
        b = M.emu_call(CASES[name], order=2, seed=99, flags=0)
        assert a[0] == 0 and (a[1] == b[1]).all() and a[2:] == b[2:]


def test_four_passes():
    T = CASES["w3_n20001"]
    expect = M.want("w3_n20001", 0)[0]
    n, nb, nw = C.c_int64(), C.c_int64(), C.c_int64()
    buf = np.zeros(len(expect), np.uint8)
    arr = (C.c_char_p * len(T.L.names))(*T.L.names)
    p = lambda x: C.c_void_p(x.ctypes.data)      # noqa: E731
    rc = M.emu_lib().mtext_emu_door(C.c_int(0), C.c_uint64(1), C.c_int64(len(T.L.names)), p(T.L.seg), arr, p(T.L.s), p(T.L.f), p(T.vals), C.c_int32(3), None, None,
                                    C.c_uint32(0), None, p(buf), C.c_int64(len(expect)), C.byref(nb), C.byref(nw), C.byref(n))
    assert rc == 0 and n.value == 4 and buf.tobytes() == expect      # cells, mode, scan, emit
