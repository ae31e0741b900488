"""The passes of csrc/wt_hist.h run through the CPU emulator (tests/hist_emu.cpp: the product's own door over a launcher that
runs the workgroups forwards, backwards or shuffled) and the product's host sweep, on every fixture and on the seam cases of
hist_model.seam_cases: the three orders give the same bits, and those bits are the model's."""
import functools

import numpy as np
import pytest

import hist_model as M

SEAMS = M.seam_cases()


def _door(order, seed=7):
    return lambda L, w, flags=0, given=None, base=None, dtype=np.float64: M.emu_door(L, w, order, seed, flags, given, base, dtype)


def _host(L, w, flags=0, given=None, base=None, dtype=np.float64):
    return M.host_sweep(M.Lists(L.seg, L.row, L.n_rows, L.s, L.f, L.v.astype(dtype).astype(np.float64)), w, flags, given, base)


DOORS = {"forwards": _door(0), "backwards": _door(1), "shuffled": _door(2), "host sweep": _host}


@pytest.mark.parametrize("how", sorted(DOORS))
def test_fixtures(how):
    for c in M.fixtures():
        L, w = M.fixture_lists(c)
        rng, model = M.check_case(DOORS[how], L, w, c["name"], dtypes=(np.float64,))
        assert M.same_bits(model, M.fixture_result(c)[1]) and M.same_bits(rng, M.fixture_result(c)[0])
        # the same values rounded to float32 and widened again: the model over those
        L32 = M.Lists(L.seg, L.row, L.n_rows, L.s, L.f, L.v.astype(np.float32).astype(np.float64))
        M.check_case(DOORS[how], L32, w, (c["name"], "f32"))


def test_all_fixtures_in_one_call_with_a_row_per_fixture_row():
    L, rows = M.all_fixtures_as_one()
    for how in sorted(DOORS):
        M.check_case(DOORS[how], L, 10, how, dtypes=(np.float64,))


@pytest.mark.parametrize("name", sorted(SEAMS))
def test_seams_in_every_order(name):
    L, w = SEAMS[name]
    for how in sorted(DOORS):
        M.check_case(DOORS[how], L, w, (name, how))


def test_the_table_cuts_a_stretch_of_one_row_into_shares():
    """3 S + 1 runs of one row are four workgroups whatever the segments inside; one more launch for every pass."""
    import ctypes as C
    S = M.constants()["SHARE"]
    L, w = SEAMS["rows"]
    n = C.c_int64()
    v = L.v
    r2, out = np.zeros(2), np.zeros((L.n_rows, w))
    rc = M.emu_lib().hist_emu_door(C.c_int(0), C.c_uint64(1), C.c_int64(len(L.row)), M._p(L.seg), M._p(L.row), C.c_int32(L.n_rows), M._p(L.s), M._p(L.f),
                                   M._p(v), C.c_int(1), C.c_int32(w), C.c_uint32(0), M._p(r2), M._p(out), C.byref(n))
    assert rc == 0 and n.value == 3                 # range, bins, finish
    assert S == M.constants()["BLOCK"] * M.constants()["RUNS_PER_LANE"]


@pytest.mark.parametrize("how", sorted(DOORS))
def test_split_lists_compose(how):
    S = M.constants()["SHARE"]
    L, w = SEAMS["rows"]
    M.check_split(DOORS[how], L, w, [S - 3, S + 1, 4 * S + 70], how)
    L, w = SEAMS["wave_of_columns_w%d" % (M.constants()["LDS_WIDTH"] + 1)]
    M.check_split(DOORS[how], L, w, [1, 2, S], how)


@pytest.mark.parametrize("how", sorted(DOORS))
def test_refusals_write_nothing(how):
    M.check_refusals(DOORS[how], 1)
