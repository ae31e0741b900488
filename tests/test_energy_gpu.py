"""Energy spectra on the device (csrc/wt_energy.hip: wtamd_runs_energy) against the exact values of the rule recorded by
tests/golden/make_energy_golden.py (mpmath at 60 digits; tests/test_energy_model.py pins them to the compiled reference within
the reference's own bound): real and im within 2^-53 (48 + n) S, NaN exactly where the model says NaN, f32 and f64 input of the
same values with the same bits, the same call twice with the same bits.  The seam sizes come from the header's constants
(energy_model.constants)."""
import numpy as np
import pytest

import energy_model as M

pytestmark = pytest.mark.gpu

SEAMS = M.seam_cases()
VALUES = M.seam_values()
ERR_ARG = 1


def _door(L, lam, seg_base=None, dtype=np.float64):
    from wiggletools_amd import engine
    from wiggletools_amd.runlists import RunLists
    rl = RunLists(L.n_seg, 1, L.seg, L.s, L.f, L.v.astype(dtype), [0.0])
    return engine._energy_door(rl, lam, seg_base)


def _seam_exact(name):
    r = VALUES[name]
    return np.array([[M._num(a), M._num(b)] for a, b in r["exact"]], np.float64).reshape(-1, 2), (M._num(r["S"]) if r["S"] is not None else float("nan"))


def test_fixtures_case_by_case():
    for c in M.fixtures():
        L, lam = M.fixture_lists(c), M.fixture_wavelengths(c)
        rc, out, end = _door(L, lam)
        assert rc == 0 and end == M.bases(L)[1], (c["name"], rc, end)
        M.check_close(out, M.fixture_exact(c), len(L.s), M._num(c["S"]), c["name"])
        # the same values rounded to float32: as f32 and as f64 input, the same bits
        L32 = L.as_f32()
        rc_a, a, _ = _door(L32, lam, None, np.float32)
        rc_b, b, _ = _door(L32, lam, None, np.float64)
        assert rc_a == rc_b == 0 and M.same_bits(a, b), c["name"]
        if np.array_equal(L32.v, L.v, equal_nan=True):
            assert M.same_bits(a, out), c["name"]


@pytest.mark.parametrize("name", sorted(SEAMS))
def test_seams(name):
    """Run counts 0, 1, a lane's batch +- 1, a workgroup's share - 1 / exact / + 1 and 3 shares + 1; segment boundaries inside a
    share and an empty segment between two full ones; wavelength counts 1, a chunk - 1 / exact / + 1 and two chunks + 1 with a
    repeated wavelength; wavelengths 1, 2, 3, 2^31 - 1 and one equal to a run's length; a negative start, a base of 3 10^9 given
    explicitly, a finish at WTAMD_MAX_COORD, lengths of 1 and of 2^30; NaN in the first run, in the last run of a share, and an
    infinity."""
    L, lam, sb = SEAMS[name]
    star, S = _seam_exact(name)
    rc, out, end = _door(L, lam, sb)
    assert rc == 0 and end == VALUES[name]["end_base"], (name, rc, end)
    M.check_close(out, star, len(L.s), S, name)
    rc32, out32, _ = _door(L, lam, sb, np.float32)
    assert rc32 == 0 and M.same_bits(out, out32), (name, "f32")
    rc2, again, _ = _door(L, lam, sb)
    assert rc2 == 0 and M.same_bits(out, again), (name, "the same call twice")
    lam = list(lam)
    for a in range(len(lam)):
        for b in range(a + 1, len(lam)):
            if lam[a] == lam[b]:
                assert M.same_bits(out[a], out[b]), (name, lam[a])


def test_a_wavelength_is_served_alike_in_any_company():
    K = M.constants()["KCHUNK"]
    L, lam, sb = SEAMS["wavelengths_%d" % (2 * K + 1)]
    _, full, _ = _door(L, lam, sb)
    for k in (0, K - 1, K, len(lam) - 1):
        _, one, _ = _door(L, [lam[k]], sb)
        assert M.same_bits(one[0], full[k]), lam[k]


def test_a_split_list_chains_through_end_base():
    S = M.constants()["SHARE"]
    L, lam, _ = SEAMS["segments"]
    star, W = _seam_exact("segments")
    M.check_split(_door, L, lam, star, W, [S - 3, S + 1], "segments")


def test_seg_base_null_is_the_rule_given_explicitly():
    L, lam, _ = SEAMS["segments"]
    rc, a, ea = _door(L, lam, None)
    rc2, b, eb = _door(L, lam, M.bases(L)[0])
    assert rc == rc2 == 0 and M.same_bits(a, b) and ea == eb


def test_energy_runlists_has_one_spectrum_per_track():
    from wiggletools_amd import engine
    from wiggletools_amd.runlists import RunLists
    c = [c for c in M.fixtures() if len(c["chroms"]) == 3 and not c["seek"] and not np.isnan(M.fixture_exact(c)).any()][0]
    L, lam = M.fixture_lists(c), M.fixture_wavelengths(c)
    # two tracks: the fixture (the union of its child), and the same with its values doubled; chromosome-major segments
    order = []
    for s, f, v in L.segments():
        order += [(s, f, v), (s, f, 2 * v)]
    two = M.Lists.from_segments(order)
    rl = RunLists(3, 2, two.seg, two.s, two.f, two.v, [0.0, 0.0])
    e = engine.energy_runlists(rl, lam)
    star = M.fixture_exact(c)
    t = M.door_bound(len(L.s), M._num(c["S"]))
    assert (np.abs(e[0] - M.energy(star)) <= M.energy_bound(star, t)).all()
    assert (np.abs(e[1] - 4 * M.energy(star)) <= 4 * M.energy_bound(star, t)).all()


def test_refusals_return_err_arg_and_write_nothing():
    """Every refusal is decided by the argument checks or by the first pass, before anything is written."""
    M.check_refusals(_door, ERR_ARG)
    from wiggletools_amd import _lib
    assert b"wtamd_runs_energy" in _lib.lib().wtamd_last_error()


def test_the_host_entry_gives_the_same_bits():
    from wiggletools_amd import _lib
    for name in ("segments", "far_base", "wavelengths_%d" % (M.constants()["KCHUNK"] + 1)):
        L, lam, sb = SEAMS[name]
        rc, dev, end = _door(L, lam, sb)
        rc2, host, end2 = M.call(_lib.lib().wtamd_runs_energy_host, [], L, lam, sb, None)
        assert rc == rc2 == 0 and M.same_bits(dev, host) and end == end2, name
    M.check_refusals(lambda L, lam, sb, dt: M.call(_lib.lib().wtamd_runs_energy_host, [], M.Lists(L.seg, L.s, L.f, L.v.astype(dt)), lam, sb, None), ERR_ARG)
