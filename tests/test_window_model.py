"""The window operators off the device: the per-pop model of tests/window_model.py pinned to every value recorded from the compiled
reference (tests/golden/window_fixtures.json), and the plain-C++ passes and host sweeps of csrc/wt_window.h (tests/window_emu.cpp
over tests/emu/runs_launcher.h) against the model, in natural and shuffled block order, at every seam of the header's constants."""
import numpy as np
import pytest

import window_model as M

FIXTURES = M.load_fixtures()
BIN_SEAMS = M.bin_seams()
SMOOTH_SEAMS = M.smooth_seams()


def _model(op, case, w, default):
    return M.bin(case.chroms, w, default) if op == "bin" else M.smooth(case.chroms, w)


def test_the_model_gives_every_recorded_value_bit_for_bit():
    n = seeks = 0
    for c in FIXTURES:
        case, default, w = M.fixture_case(c)
        for op in ("bin", "smooth"):
            for rec, sub in [(c[op], case)] + ([(c[op]["seek"], M.seek_child(case, c[op]["seek"]["chrom"], c[op]["seek"]["lo"], c[op]["seek"]["hi"]))]
                                               if "seek" in c[op] else []):
                rows, model = M.recorded(rec), _model(op, sub, w, default)
                assert [r[:3] for r in rows] == [r[:3] for r in model], (c["name"], op)
                assert M.same_bits([r[3] for r in rows], [r[3].float() for r in model]), (c["name"], op)
                n += len(rows)
                seeks += rec is not c[op]
        d = c["bin"]["default"]
        assert M.same_bits([M._num(d)], [default * w]) and M.same_bits([M._num(c["smooth"]["default"])], [default]), c["name"]
    assert n > 30000 and seeks >= 2


def test_every_recorded_bin_lies_on_the_grid():
    """:990-996: continuing at the last finish and realigning land on the same grid, bins of 1 + k w; a bin is there iff a run
    intersects it, in order, and none is merged."""
    for c in FIXTURES:
        case, _, w = M.fixture_case(c)
        rows = M.recorded(c["bin"])
        assert all((r[1] - 1) % w == 0 and r[2] == r[1] + w for r in rows), c["name"]
        for g, (s, f, _) in enumerate(case.chroms):
            want = sorted({k for a, b in zip(s.tolist(), f.tolist()) for k in range((a - 1) // w, (b - 2) // w + 1)})
            assert [(r[1] - 1) // w for r in rows if r[0] == g] == want, (c["name"], g)


def test_the_recorded_cases_are_the_ones_asked_for():
    seen = {"short_w": 0, "short_h": 0, "nan": 0, "gaps": set(), "edge": 0, "first": set()}
    for c in FIXTURES:
        case, default, w = M.fixture_case(c)
        h = w // 2
        for s, f, v in case.chroms:
            ext = int(f[-1] - s[0])
            seen["short_w"] += ext < w
            seen["short_h"] += ext < h
            seen["nan"] += bool(np.isnan(v).any())
            seen["gaps"] |= {int(x) - w for x in (s[1:] - f[:-1]) if abs(int(x) - w) <= 1}
            seen["edge"] += int(((f - 1) % w == 0).sum())
        s0 = int(case.chroms[0][0][0])
        seen["first"].add("1" if s0 == 1 else "h" if s0 == h else "h+1" if s0 == h + 1 else "far")
    assert seen["short_w"] and seen["short_h"] and seen["nan"] >= 10 and seen["gaps"] == {-1, 0, 1} and seen["edge"] > 50, seen
    assert seen["first"] == {"1", "h", "h+1", "far"}, seen
    assert {c["width"] for c in FIXTURES} == set(M.WIDTHS)


@pytest.mark.parametrize("order", [0, 2])
def test_emulated_passes_on_every_fixture(order):
    for c in FIXTURES:
        case, default, w = M.fixture_case(c)
        for dt in (np.float32, np.float64):
            rc, n, got = M.emu_bin(case, w, default, dt, order=order, seed=3)
            assert rc == M.OK, c["name"]
            M.check_exact(got, M.bin(case.chroms, w, default), len(case.chroms), (c["name"], "bin"))
            rc, n, got = M.emu_smooth(case, w, dt, order=order, seed=3)
            assert rc == M.OK, c["name"]
            M.check_exact(got, M.smooth(case.chroms, w), len(case.chroms), (c["name"], "smooth"))


@pytest.mark.parametrize("name", sorted(BIN_SEAMS))
def test_emulated_bin_seams(name):
    case, w = BIN_SEAMS[name]
    for default in M.DEFAULTS:
        model = M.bin(case.chroms, w, default)
        for order in (0, 1, 2):
            rc, n, got = M.emu_bin(case, w, default, np.float32, order=order, seed=5)
            assert rc == M.OK and n == len(model), name
            M.check_exact(got, model, len(case.chroms), name)
        rc, got = M.host_sweep(case, w, default)
        assert rc == M.OK
        M.check_exact(got, model, len(case.chroms), (name, "host"))


@pytest.mark.parametrize("name", sorted(SMOOTH_SEAMS))
def test_emulated_smooth_seams(name):
    case, w = SMOOTH_SEAMS[name]
    model = M.smooth(case.chroms, w)
    for order in (0, 2):
        rc, n, got = M.emu_smooth(case, w, np.float32, order=order, seed=5)
        assert rc == M.OK and n == len(model), name
        M.check_exact(got, model, len(case.chroms), name)
    rc, got = M.host_sweep(case, w)
    assert rc == M.OK
    M.check_exact(got, model, len(case.chroms), (name, "host"))


def test_a_clipped_smooth_is_the_slice_of_the_whole():
    c = M.constants()
    case, w = SMOOTH_SEAMS["extent%d" % (c["STRIP"] * 256 + 1)]
    rc, n, (oseg, os_, of, ov) = M.emu_smooth(case, w)
    assert rc == M.OK
    for lo, hi in ((1, 60), (47, 48), (60, c["STRIP"] * 256 + 70), (5000, 6000), (3, 2 ** 31 - 1)):
        rc, k, (cseg, cs, cf, cv) = M.emu_smooth(case, w, clip=(lo, hi), order=2, seed=1)
        assert rc == M.OK
        keep = (os_[:n] >= lo) & (os_[:n] < hi)
        assert k == keep.sum() and np.array_equal(cs[:k], os_[:n][keep]) and np.array_equal(cf[:k], of[:n][keep]) and M.same_bits(cv[:k], ov[:n][keep]), (lo, hi)
        rc, host = M.host_sweep(case, w, clip=(lo, hi))
        assert rc == M.OK and np.array_equal(host[1], cs[:k]) and M.same_bits(host[3], cv[:k]), (lo, hi)


def test_float_case_within_the_derived_bounds():
    case = M.float_case()
    for w in (3, 10, 1000):
        rc, n, got = M.emu_bin(case, w, 1.5, np.float32, order=2, seed=9)
        assert rc == M.OK
        M.check_bin_bound(got, M.bin(case.chroms, w, 1.5), 1, ("float bin", w))
        rc, host = M.host_sweep(case, w, 1.5)
        assert rc == M.OK and M.same_bits(host[3], got[3][:n])
    for w in (3, 10, 100):
        rc, n, got = M.emu_smooth(case, w, np.float32, order=2, seed=9)
        assert rc == M.OK
        M.check_smooth_bound(got, M.smooth(case.chroms, w), case, w, ("float smooth", w))
        rc, host = M.host_sweep(case, w)
        assert rc == M.OK and M.same_bits(host[3], got[3][:n])


def test_refusals_and_capacity_leave_the_output_untouched():
    case, w = BIN_SEAMS["segments"]
    untouched = lambda got: (got[1] == -1).all() and (got[2] == -1).all() and (got[3] == -1.0).all()      # noqa: E731
    for what, bad, width in M.refusals(case):
        rc, n, got = M.emu_bin(bad, width, 1.5, capacity=4000)
        assert rc == M.ERR_ARG and untouched(got), what
        rc, n, got = M.emu_smooth(bad, width, capacity=4000)
        assert rc == M.ERR_ARG and untouched(got), what
        if width >= 2 and what != "past INT32_MAX":             # (the sweeps' callers size their output from the input)
            assert M.host_sweep(bad, width, 1.5)[0] == M.ERR_ARG and M.host_sweep(bad, width)[0] == M.ERR_ARG, what
    need = len(M.bin(case.chroms, w, 0.0))
    rc, n, got = M.emu_bin(case, w, 0.0, capacity=need - 1)
    assert rc == M.ERR_CAPACITY and n == need and untouched(got)
    need = len(M.smooth(case.chroms, w))
    rc, n, got = M.emu_smooth(case, w, capacity=need - 1)
    assert rc == M.ERR_CAPACITY and n == need and untouched(got)
    assert need <= M.smooth_capacity(case, w) and len(M.bin(case.chroms, w, 0.0)) <= M.bin_capacity(case, w)


def test_dropin_window_iterators_on_the_host():
    """wtamd_BinIterator and wtamd_SmoothIterator in the emulated drop-in library (no HIP unit: the weak references to the device
    doors are null and the iterators sweep on the host): by pop, in blocks, after a seek, under a SumReduction, over an
    overlapping child, and over a chromosome that starts below 1."""
    import window_dropin
    from emu import build as emu_build
    window_dropin.check_dropin(window_dropin.DropIn(emu_build.build_dropin()), FIXTURES)


def test_the_window_seams_put_exactly_that_many_owners_under_the_first_tile():
    c = M.constants()
    for n in (c["WINDOW"], c["WINDOW"] + 1):
        case, w = BIN_SEAMS["window%d" % n]
        s, f = case.s.astype(np.int64), case.f.astype(np.int64)
        last = (f - 2) // w
        first = np.maximum((s - 1) // w, np.concatenate([[-1], last[:-1]]) + 1)
        cum = np.concatenate([[0], np.cumsum(last - first + 1)])            # output bins before the bins run i owns
        owner = lambda o: int(np.searchsorted(cum, o, side="right")) - 1      # noqa: E731
        assert cum[-1] > c["TILE"] and owner(c["TILE"] - 1) - owner(0) + 1 == n
