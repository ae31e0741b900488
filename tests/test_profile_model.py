"""Region profiles (`profile` / `profiles`) on the CPU: the per-base-pair Fraction model (tests/profile_model.py) against rows
recorded from the compiled reference's ProfileMultiplexer (tests/golden/profile_fixtures.json); its closed form against the
literal rule; the passes of csrc/wt_profile.h run workgroup by workgroup in shuffled order (tests/profile_emu.cpp) and the
header's host sweep against the model; the drop-in built without HIP units.  The same cases run on the device in
tests/test_profile_gpu.py."""
import numpy as np
import pytest

import apply_model as AM
import profile_model as M


@pytest.fixture(scope="module")
def fixtures():
    return M.load_fixtures()


def test_round_is_c_round():
    x = np.array([0.0, 0.49999999999999994, 0.5, 0.5000000000000001, 1.5, 2.5, 2.4999999999999996, 3.5, 1e6 + 0.5, 4503599627370495.5, 2.0 ** 52 + 1])
    assert M.cround_vec(x).tolist() == [M.cround(v) for v in x] == [0.0, 0.0, 1.0, 1.0, 2.0, 3.0, 2.0, 4.0, 1000001.0, 4503599627370496.0, 2.0 ** 52 + 1]
    rng = np.random.default_rng(1)
    for L, W in ((6, 1), (6, 3), (14, 7), (999983, 1000), (3, 4099), (1 << 30, 777)):
        i = np.unique(np.concatenate([np.arange(0, min(L, 2000) + 1), rng.integers(0, L + 1, 2000)])).astype(np.float64)
        p = i * (W / float(L))
        assert M.cround_vec(p).tolist() == [M.cround(v) for v in p]


def test_the_worked_examples():
    cases = M.rounding_cases()
    case, W = cases["ones"]
    assert [float(b.s) for b in M.literal(*case.data[0], 10, 30, W, 0.0)] == [3.0, 5.0, 5.0, 5.0]
    case, W = cases["worked"]
    assert [float(b.s) for b in M.literal(*case.data[0], 100, 120, W, 0.5)] == [2.5, 4.5, 3.0, 5.0]


def test_model_equals_the_compiled_reference(fixtures):
    """Every recorded row against the literal model by M.check_row (bit for bit where the bin is exact), and the running sum
    against the concatenated terms.  Where the reference's group seek cut the dataset short (apply_model.reference_stops) the
    model is given the dataset cut there: that departure is documented in include/wiggletools_amd.h."""
    assert len(fixtures) >= 120
    regimes, widths, inexact, total, bitten, exact_cases = set(), set(), 0, 0, 0, 0
    for c in fixtures:
        case, default, W = M.fixture_case(c)
        default = float(np.float32(default))                # (apply.c:42; 0, 1.5 and NaN are themselves in float)
        stops = AM.reference_stops(case)
        assert c["start"] == case.rs.tolist() and c["finish"] == case.rf.tolist(), c["name"]
        assert c["chrom"] == np.repeat(np.arange(len(case.regions)), np.diff(case.rseg)).tolist(), c["name"]
        rec = M.recorded_rows(c)
        assert rec.shape == (len(case.rs), W) and int((case.rf.astype(np.int64) - case.rs).max()) < 10 ** 6
        widths.add(W)
        rows, i, all_exact = [], 0, True
        for (s, f, v), (rs_, rf_) in zip(case.data, case.regions):
            for rs, rf in zip(rs_.tolist(), rf_.tolist()):
                keep = s < stops[i]
                bitten += bool((f[s < rf] > stops[i]).any())
                bins = M.literal(s[keep], np.minimum(f[keep], stops[i]), v[keep], rs, rf, W, default)
                M.check_row(rec[i], bins, (c["name"], i))
                rows.append(bins)
                L = rf - rs
                regimes.add("L<W" if L < W else "L==W" if L == W else "W<L<2W" if L < 2 * W else "L==2W" if L == 2 * W else "L>2W")
                inexact += sum(not b.exact for b in bins)
                all_exact = all_exact and all(b.exact for b in bins)
                total += W
                i += 1
        exact_cases += all_exact
        M.check_row(np.array([float("nan") if x is None else x for x in c["sum"]]), M.column_sums(rows), (c["name"], "sum"))
    assert regimes == {"L<W", "L==W", "W<L<2W", "L==2W", "L>2W"} and widths == {1, 2, 3, 7, 10, 64, 100}
    assert inexact <= 0.40 * total and exact_cases > 0, (inexact, total, exact_cases)
    assert bitten > 0


def test_closed_form_equals_the_literal_rule(fixtures):
    for c in fixtures:
        case, default, W = M.fixture_case(c)
        lit, clo = M.Expected(case, M.literal), M.Expected(case, M.closed)
        for a, b in zip(lit.rows(W, default), clo.rows(W, default)):
            assert M.same_bins(a, b), c["name"]
    for name, (case, W) in sorted(M.rounding_cases().items()):
        if int((case.rf.astype(np.int64) - case.rs).max()) > 5000:
            continue
        for default in M.DEFAULTS:
            for a, b in zip(M.Expected(case, M.literal).rows(W, default), M.Expected(case, M.closed).rows(W, default)):
                assert M.same_bins(a, b), (name, default)
    # ... and at one long region, once
    case, W = M.rounding_cases()["L999983_W1000"]
    sub = case.subset([0])
    assert M.same_bins(M.Expected(sub, M.literal).rows(W, 1.5)[0], M.Expected(sub, M.closed).rows(W, 1.5)[0])


def _check_emu(case, W, what, defaults=M.DEFAULTS, exp=None):
    exp = exp or M.Expected(case)
    for default in defaults:
        got = []
        for k, (order, dt) in enumerate(((0, np.float64), (2, np.float32), (2, np.float64))):
            rc, out = M.emu_case(case, W, default, 0, dt, order=order, seed=17 + k)
            assert rc == M.OK, what
            got.append(out.copy())
        exp.check(got[0], W, default, what)
        assert M.same_rows(got[0], got[1]) and M.same_rows(got[1], got[2]), what       # two shuffles, either width: the same bits
        rc, host = M.host_sweep(case, W, default)
        assert rc == M.OK and M.same_rows(host, got[0]), what + " host sweep"
        # the sum: the same bits at every batch size, and the host's when there is one segment
        sums = []
        for batch in (0, 1, 2, 8):
            rc, out = M.emu_case(case, W, default, M.SUM, np.float32, order=2, seed=5, batch=batch)
            assert rc == M.OK, what
            sums.append(out.copy())
        exp.check(sums[0], W, default, what + " sum", sum_mode=True)
        assert all(M.same_rows(sums[0], x) for x in sums[1:]), what + " sum by batch"
        if len(case.seg) == 2:
            rc, out = M.host_sum(case, W, default)
            assert rc == M.OK and M.same_rows(out, sums[0]), what + " host sum"


def test_emulated_passes_and_host_sweep_on_the_fixtures(fixtures):
    for c in fixtures:
        case, default, W = M.fixture_case(c)
        _check_emu(case, W, c["name"], defaults=(default,))
    one, _ = AM.all_fixtures_in_one(fixtures)
    for W in (3, 64):
        _check_emu(one, W, "all", defaults=(1.5,))


ROUNDING = M.rounding_cases()
REGIMES = M.regime_cases()


@pytest.mark.parametrize("name", sorted(ROUNDING))
def test_emulated_passes_at_the_rounding_seams(name):
    case, W = ROUNDING[name]
    _check_emu(case, W, name)


@pytest.mark.parametrize("name", sorted(REGIMES))
def test_emulated_passes_at_the_regime_seams(name):
    case, W = REGIMES[name]
    _check_emu(case, W, name, defaults=(1.5,) if name.startswith("regions") else M.DEFAULTS)


def _runs_under_bin0(case, W):
    """Runs that meet the positions of bin 0 of the case's first region."""
    rs, rf = int(case.rs[0]), int(case.rf[0])
    L = rf - rs
    r = M.cround_vec(np.arange(L + 1, dtype=np.float64) * (W / float(L)))
    b1 = min(int(np.searchsorted(r, 1, side="left")), L)
    return int(np.searchsorted(case.s, rs + b1, side="left")) - int(np.searchsorted(case.f, rs, side="right"))


def test_seam_cases_are_what_they_claim():
    c = M.constants()
    S, WV, T, WIN = c["SMALL"], c["WAVE"], c["TILE"], c["WINDOW"]
    under = {_runs_under_bin0(*REGIMES[k]) for k in REGIMES if k.startswith("bin")}
    for n in (S - 1, S, S + 1, WV - 1, WV, WV + 1, S * WV - 1, S * WV, S * WV + 1, 3 * S * WV + 5):
        assert n in under, (n, sorted(under))
    for n in (T - 1, T, T + 1, 3 * T + 5):
        assert len(REGIMES["regions%d" % n][0].rs) == n
    for w in (WIN, WIN + 1):
        k = REGIMES["window%d" % w][0]
        assert np.searchsorted(k.s, k.rf.max(), side="left") - np.searchsorted(k.f, k.rs[0], side="right") == w and len(k.rs) <= T
    k = REGIMES["segments"][0]
    assert {(len(d[0]) > 0, len(r[0]) > 0) for d, r in zip(k.data, k.regions)} == {(True, True), (True, False), (False, True), (False, False)}
    assert {"L<W", "L==W", "L==W+1", "L==W-1", "L==2W", "L==2W+1", "L==2W-1"} <= {
        "L<W" if L < W - 1 else "L==W-1" if L == W - 1 else "L==W" if L == W else "L==W+1" if L == W + 1 else "L==2W-1" if L == 2 * W - 1 else
        "L==2W" if L == 2 * W else "L==2W+1" if L == 2 * W + 1 else "other" for L, W in M.ROUNDING}
    # the edges, spelled out (W = 4, default 1.5)
    k, W = REGIMES["edges_W4"]
    rows = {(int(a), int(b)): [float(x.s) for x in row] for a, b, row in zip(k.rs, k.rf, M.Expected(k, M.literal).rows(W, 1.5))}
    assert rows[(1, 5)] == [0.375] * 4                      # no data: ONE sample of the default over round(0) .. round(4 c)
    assert rows[(12, 18)] == [1.0, 2.0, 1.0, 2.0]           # inside one run, L = 6: round(i 4 / 6) = 0 1 1 2 3 3
    assert rows[(60, 900)] == [0.375] * 4                   # behind the last run
    assert rows[(20, 25)] == [0.0] * 4                      # a NaN run: covered, skipped
    assert rows[(20, 30)] == [0.0, 0.0, 0.75, 0.75]         # ... and the gap behind it: one sample over bins 2 and 3
    assert rows[(41, 100)] == [1.5, 25.5, 0.5, 0.5]         # gap [0,9) in bin 0; the run's 10 bp in bin 1; gap [19,59) over bins 1 .. 3


def test_a_region_alone_equals_the_region_inside_the_full_call():
    rng = np.random.default_rng(5)
    c = M.constants()
    for name in ("regions%d" % (3 * c["TILE"] + 5), "bin%d_float" % (3 * c["SMALL"] * c["WAVE"] + 5), "segments", "window%d" % c["WINDOW"]):
        case, W = REGIMES[name]
        rc, full = M.emu_case(case, W, 1.5, 0, np.float32, order=2, seed=1)
        assert rc == M.OK
        for i in np.unique(np.concatenate([[0, len(case.rs) - 1], rng.integers(0, len(case.rs), 8)])):
            rc, alone = M.emu_case(case.subset([i]), W, 1.5, 0, np.float32, order=2, seed=2)
            assert rc == M.OK and M.same_rows(alone, full[i:i + 1]), (name, i)
        idx = np.arange(0, len(case.rs), 3)
        rc, part = M.emu_case(case.subset(idx), W, 1.5, 0, np.float32, order=2, seed=3)
        assert rc == M.OK and M.same_rows(part, full[idx]), name


def test_the_sum_is_one_tree_whatever_the_batch():
    case = M.float_case()
    exp = M.Expected(case)
    for W in (1, 5):
        sums = []
        for batch in (0, 1, 4, 64, 256):
            rc, out = M.emu_case(case, W, 1.5, M.SUM, order=2, seed=batch, batch=batch)
            assert rc == M.OK
            sums.append(out.copy())
        assert all(M.same_rows(sums[0], x) for x in sums[1:])
        exp.check(sums[0], W, 1.5, "float sum", sum_mode=True)
        rc, host = M.host_sum(case, W, 1.5)
        assert rc == M.OK and M.same_rows(host, sums[0])
        # R = batch - 1, batch, batch + 1 regions
        for n in (63, 64, 65):
            sub = case.subset(np.arange(n))
            got = [M.emu_case(sub, W, 1.5, M.SUM, order=2, seed=1, batch=b)[1].copy() for b in (64, 0, 2)]
            assert M.same_rows(got[0], got[1]) and M.same_rows(got[0], got[2])
            M.Expected(sub).check(got[0], W, 1.5, "float sum %d" % n, sum_mode=True)


def test_emulated_refusals_leave_the_output_untouched():
    case, W = REGIMES["segments"]
    assert M.emu_case(case, W, 0.0)[0] == M.OK
    for what, kw in M.refusals(case):
        kw = dict(kw)
        w, flags = kw.pop("W", W), kw.pop("flags", 0)
        rc, out = M.emu_case(M.altered(case, **kw), w, 0.0, flags, order=2, seed=9)
        assert rc == M.ERR_ARG and (out == -1.0).all(), what


def test_dropin_profile_multiplexer_on_the_host(fixtures):
    """wtamd_ProfileMultiplexer in the emulated drop-in library (no HIP unit: the weak reference to the device door is null and
    the Multiplexer sweeps on the host): by pop, under SelectReduction, after a seek, over a MeanReduction."""
    import profile_dropin
    from emu import build as emu_build
    profile_dropin.check_dropin(profile_dropin.DropIn(emu_build.build_dropin()), fixtures)
