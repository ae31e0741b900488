"""The passes of csrc/wt_read.h run through the CPU emulator (tests/read_emu.cpp: the product's own door over a launcher that
runs the workgroups forwards, backwards or shuffled) and the product's host sweep, on every case of read_model.cases(): record
for record, bit for bit, the Python model's reading, which tests/golden/make_read_golden.py holds to the compiled reference's."""
import ctypes as C

import numpy as np
import pytest

import read_model as M

CASES = M.cases()
DOORS = {"forwards": M.host_door("emu", 0), "backwards": M.host_door("emu", 1), "shuffled": M.host_door("emu", 2)}
HOST = M.host_door("host")


@pytest.mark.parametrize("how", sorted(DOORS))
def test_every_case_is_the_model_s_reading(how):
    for name, (data, flags) in CASES.items():
        M.check_reading(DOORS[how](data, flags), data, flags, None, (name, how))


def test_the_host_sweep_gives_the_same_records_with_the_slow_values_read():
    for name, (data, flags) in CASES.items():
        M.check_reading(HOST(data, flags), data, flags, None, (name, "host sweep"), host_values=True)


@pytest.mark.parametrize("how", sorted(DOORS))
def test_the_slow_list_is_the_model_s(how):
    """The rule is deterministic: the same numerals are slow, no tolerance and no cap."""
    for name in ("values", "long_number"):
        data, flags = CASES[name]
        m = M.check_reading(DOORS[how](data, flags), data, flags, None, (name, how))
        assert m.counts["n_slow"] >= 3


@pytest.mark.parametrize("how", sorted(DOORS))
def test_cut_texts_chain_through_the_state(how):
    door = DOORS[how]
    for name in ("mixed_257", "section_three_tiles", "same_chrom_headers", "bedgraph_after_fixed", "chrom_changes", "short_lines", "header_ends_tile",
                 "values", "bed_257", "no_final_newline_fixed", "coordinates"):
        data, flags = CASES[name]
        M.check_chained(door, data, flags, (name, how))


@pytest.mark.parametrize("how", ["forwards", "shuffled", "host sweep"])
def test_refusals_write_nothing(how):
    M.check_refusals(DOORS.get(how, HOST))


@pytest.mark.parametrize("how", ["forwards", "backwards", "host sweep"])
def test_one_entry_short_is_refused_with_the_counts_needed(how):
    data, flags = CASES["values"]
    door = DOORS.get(how, HOST)
    if how == "host sweep":
        m = M.read(data, flags)
        out = door(data, flags, capacity=m.counts["n_runs"] - 1)
        assert out["rc"] == M.ERR_CAPACITY and out["counts"] == m.counts and M.nothing_written(out)
        return
    M.check_capacities(door, data, flags, how)


@pytest.mark.parametrize("how", sorted(DOORS) + ["host sweep"])
def test_an_empty_call_leaves_the_state_alone(how):
    M.check_empty(DOORS.get(how, HOST))


def test_text_at_every_alignment():
    data, flags = CASES["mixed_257"]
    for off in range(16):
        M.check_reading(DOORS["forwards"](data, flags, offset=off), data, flags, None, off)


def test_six_launches_and_the_documented_scratch():
    data, flags = CASES["mixed_257"]
    m = M.read(data, flags)
    n = C.c_int64()
    st, cn = M.State(), M.Counts()
    a = [np.zeros(m.counts["n_runs"] + 1, np.int64) for _ in range(8)]
    p = lambda x: C.c_void_p(x.ctypes.data)      # noqa: E731
    rc = M.emu_lib().read_emu_door(C.c_int(0), C.c_uint64(1), data, C.c_int64(len(data)), C.c_uint32(flags), C.byref(st), p(a[0]), p(a[1]), p(a[2]),
                                   C.c_int64(m.counts["n_runs"]), p(a[3]), p(a[4]), p(a[5]), C.c_int64(m.counts["n_seg"]), p(a[6]), p(a[7]),
                                   C.c_int64(m.counts["n_slow"]), C.byref(cn), C.byref(n))
    assert rc == 0 and n.value == 6              # lines, scan, count, scan2, write, state
    assert [M.emu_lib().read_sizes(k) for k in range(4)] == [544, 64, 112, M.TILE]


def test_the_number_parser_on_the_cases():
    for tok in M.NUMBERS + [b"", b"-", b".", b"e5", b"1e", b"1e+", b"--1", b"1.2.3", b"0x10", b"1e1234", b"infinity", b"Inf", b"+1", b"1 ", b"1.e5"]:
        assert M.number_c(tok) == M.number(tok), tok
    for tok in M.fuzz_numerals(20000):
        assert M.number_c(tok) == M.number(tok), tok
