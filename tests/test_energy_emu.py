"""The passes of csrc/wt_energy.h run through the CPU emulator (tests/energy_emu.cpp: the product's own door over a launcher that
runs the workgroups forwards, backwards or shuffled) and the product's host sweep, on every fixture and on the seam cases of
energy_model.seam_cases: within the door's bound of the recorded exact values, the three orders with the same bits, f32 and
f64 input of the same values with the same bits, every refusal without a write."""
import numpy as np
import pytest

import energy_model as M

SEAMS = M.seam_cases()
VALUES = M.seam_values()


def _door(order, seed=7):
    return lambda L, lam, sb=None, dtype=np.float64: M.emu_door(L, lam, sb, dtype, order, seed)


DOORS = {"forwards": _door(0), "backwards": _door(1), "shuffled": _door(2), "host sweep": M.host_sweep}


def _seam_exact(name):
    r = VALUES[name]
    return np.array([[M._num(a), M._num(b)] for a, b in r["exact"]], np.float64).reshape(-1, 2), (M._num(r["S"]) if r["S"] is not None else float("nan"))


@pytest.mark.parametrize("how", sorted(DOORS))
def test_fixtures(how):
    for c in M.fixtures():
        L, lam = M.fixture_lists(c), M.fixture_wavelengths(c)
        rc, out, end = DOORS[how](L, lam)
        assert rc == 0 and end == M.bases(L)[1], (c["name"], rc, end)
        M.check_close(out, M.fixture_exact(c), len(L.s), M._num(c["S"]), (c["name"], how))


@pytest.mark.parametrize("name", sorted(SEAMS))
def test_seams_in_every_order(name):
    L, lam, sb = SEAMS[name]
    star, S = _seam_exact(name)
    first = None
    for how in sorted(DOORS):
        rc, out, end = DOORS[how](L, lam, sb)
        assert rc == 0 and end == VALUES[name]["end_base"] == M.bases(L, sb)[1], (name, how, rc, end)
        M.check_close(out, star, len(L.s), S, (name, how))
        rc32, out32, _ = DOORS[how](L, lam, sb, np.float32)
        assert rc32 == 0 and M.same_bits(out, out32), (name, how, "f32")
        if how != "host sweep":                             # any order of workgroups: the same bits
            first = out if first is None else first
            assert M.same_bits(out, first), (name, how)
    # a repeated wavelength: equal columns
    lam = list(lam)
    for a in range(len(lam)):
        for b in range(a + 1, len(lam)):
            if lam[a] == lam[b]:
                assert M.same_bits(first[a], first[b]), (name, lam[a])


def test_a_wavelength_is_served_alike_in_any_company():
    """The sums of a wavelength do not depend on the chunk it falls in or on the wavelengths beside it."""
    L, lam, sb = SEAMS["wavelengths_%d" % (2 * M.constants()["KCHUNK"] + 1)]
    _, full, _ = M.emu_door(L, lam, sb)
    for k in (0, M.constants()["KCHUNK"] - 1, M.constants()["KCHUNK"], len(lam) - 1):
        _, one, _ = M.emu_door(L, [lam[k]], sb)
        assert M.same_bits(one[0], full[k]), lam[k]


def test_the_passes_of_one_call():
    import ctypes as C
    L, lam, sb = SEAMS["segments"]
    n = C.c_int64()
    rc, out, end = M.call(M.emu_lib().energy_emu_door, [C.c_int(0), C.c_uint64(1)], L, lam, sb, np.float64, [C.byref(n)])
    assert rc == 0 and n.value == 3                         # last, main, final


@pytest.mark.parametrize("how", sorted(DOORS))
def test_a_split_list_chains_through_end_base(how):
    S = M.constants()["SHARE"]
    L, lam, _ = SEAMS["segments"]
    star, W = _seam_exact("segments")
    M.check_split(DOORS[how], L, lam, star, W, [S - 3, S + 1], how)


@pytest.mark.parametrize("how", sorted(DOORS))
def test_seg_base_null_is_the_rule_given_explicitly(how):
    L, lam, _ = SEAMS["segments"]
    rc, a, ea = DOORS[how](L, lam, None)
    rc2, b, eb = DOORS[how](L, lam, M.bases(L)[0])
    assert rc == rc2 == 0 and M.same_bits(a, b) and ea == eb


@pytest.mark.parametrize("how", sorted(DOORS))
def test_refusals_write_nothing(how):
    M.check_refusals(DOORS[how], 1)
