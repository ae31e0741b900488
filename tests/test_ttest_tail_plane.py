"""The t-test's tail over the (t, nu) plane, at inputs of our choosing, on every route that reaches it.

wt_ttest_tail (csrc/wt_core.h) is 2 * wt_tdist_Q under WT_EMU and wt_tdist_2Q_fast on the device, so no emulated kernel ever runs
the device's form; and on the GPU the tail was only evaluated where random data happened to land (t <= 3 or so, nu <= 98,
compared with the oracle's form at 1e-9).  Here the columns of tests/ttest_columns.py fix (t, nu) bit for bit on the device, the
emulator and the oracle; the reference is mpmath's regularised incomplete beta (40 digits) of the oracle's f64 (t, nu); the bound
is the one tests/test_tdist_fast.py::test_fast_tail_against_mpmath holds the host-compiled fast form to (ttest_columns.bound).

CPU: the host-compiled fast form on every column; the plane's regions each hold enough columns (so that it cannot shrink
unnoticed); the emulator takes the difference-array kernel on every benign float set without a patch, bit for bit the oracle.
GPU: the difference-array kernel, the general kernel (few tracks, float64, WTAMD_NO_DELTA_TTEST, the chunked plan), patched
windows (wt_patch_kernel), a redone launch, the streaming pipeline, the four strictness flags -- each within the bound, and
bit for bit the same wherever two routes ran the same columns.  A set of fewer than 3 tracks is refused there, as by the reference
(setComparisons.c:123-128): 2 v 2, 2 v 3 and 1 v 9 (nu < 2, nu = 0 / 0) are CPU cases, and the refusal is asserted on the GPU.

Measured error / bound, largest per region and route: profiles/ttest_tail_plane.txt.
"""
import ctypes as C

import numpy as np
import pytest

import ttest_columns as tc
from helpers import assert_runs_equal

MIN_PER_CLASS = 100
MAX_UNDERFLOWN = 0.10       # share of a set's columns with p_ref < 1e-290, where only the bound's absolute term decides

_ratios = {}                # (route, class) -> largest |got - p_ref| / bound seen in this session


def _ids(sizes):
    return ["%dv%d" % s for s in sizes]


def _record(route, cols, ratio):
    for name, mask in cols.classes().items():
        if mask.any():
            _ratios[(route, name)] = max(_ratios.get((route, name), 0.0), float(ratio[mask].max()))


@pytest.fixture(scope="module", autouse=True)
def _report():
    """After the module: the largest error / bound per route and region (shown with -s or -rP)."""
    yield
    routes = sorted({r for r, _ in _ratios})
    if routes:
        print("\nttest tail plane: largest |p - p_ref| / bound")
        print("%-18s" % "route" + "".join("%11s" % c for c in tc.CLASS_NAMES))
        for r in routes:
            print("%-18s" % r + "".join("%11s" % ("%.3f" % _ratios[(r, c)] if (r, c) in _ratios else "-") for c in tc.CLASS_NAMES))


def _hold(cols, values, route, what):
    """NaN exactly where the reference has it; every other column within the bound."""
    ratio = cols.ratio(values)
    _record(route, cols, ratio)
    if np.nanmax(ratio, initial=0.0) > 1.0:
        k = int(np.nanargmax(ratio))
        raise AssertionError("%s, %s: column %d (t %r, nu %r): got %r, reference %r, error / bound %.3g; %d of %d columns outside"
                             % (what, route, k, cols.t[k], cols.nu[k], float(values[k]), cols.p_ref[k], ratio[k],
                                int((ratio > 1.0).sum()), len(cols)))


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fast():
    from emu import build as emu_build
    L = C.CDLL(emu_build.build())
    L.wtemu_tdist_2q_fast.restype = C.c_double
    L.wtemu_tdist_2q_fast.argtypes = [C.c_double, C.c_double]
    return L.wtemu_tdist_2q_fast


@pytest.mark.parametrize("size", tc.SIZES + [(1, 9)], ids=_ids(tc.SIZES + [(1, 9)]))
@pytest.mark.parametrize("family", ["benign", "separated"])
def test_host_compiled_fast_form_on_the_columns(oracle, fast, size, family):
    """wt_tdist_2Q_fast compiled for the host, at every column's (t, nu): within the bound of the true value."""
    cols = tc.columns(oracle, size[0], size[1], family)
    got = np.array([fast(float(t), float(nu)) for t, nu in zip(cols.t, cols.nu)])
    _hold(cols, got, "host-compiled", "%d v %d %s" % (size + (family,)))


def test_the_plane_is_covered(oracle):
    """Every region of wt_tdist_2Q_fast holds at least 100 benign columns: the shifted series (a < 16), the y side by the textbook rule,
    the y side only by `t^2 < 9 && a <= 1000`, the x side, a > 1000, the deep tail (0 < p < 1e-100), t == 0 (1197 / 839 / 187 / 1197 /
    178 / 205 / 377 when written); no set has more than a tenth of its columns where the result underflows; nu straddles a = 16 and
    a = 1000."""
    total = dict.fromkeys(tc.CLASS_NAMES, 0)
    nus = []
    for n1, n2 in tc.SIZES:
        cols = tc.columns(oracle, n1, n2, "benign")
        assert len(cols) == tc.P_BENIGN and not cols.nan.any()
        assert np.nanmin(cols.nu) >= min(n1, n2) - 1 - 1e-9 and np.nanmax(cols.nu) <= n1 + n2 - 2 + 1e-9
        if (n1, n2) in tc.DEVICE_SIZES:             # (counted where the device can be asked: sets of >= 3 tracks)
            for name, mask in cols.classes().items():
                total[name] += int(mask.sum())
        under = float((cols.p_ref < 1e-290).mean())
        assert under <= MAX_UNDERFLOWN, (n1, n2, under)
        nus.append(cols.nu)
    assert all(v >= MIN_PER_CLASS for v in total.values()), total
    nus = np.concatenate(nus)
    for seam in (32.0, 2000.0):         # a = 16: the shift of the series; a = 1000: the side rule
        assert ((nus > 0.9 * seam) & (nus < seam)).sum() >= 10 and ((nus >= seam) & (nus < 1.1 * seam)).sum() >= 10, seam
    # the separated family reaches the tail where it is not zero (few tracks), NaN in its edge columns, and nu = n_other - 1
    for n1, n2 in tc.SIZES:
        cols = tc.columns(oracle, n1, n2, "separated")
        k = len(cols) - tc.N_EDGE
        assert cols.nan[k:k + 3].all() and not cols.nan[:k].any() and not cols.nan[k + 3:].any()
        assert np.allclose(cols.nu[k + 3:k + 6], n2 - 1, rtol=1e-12) and np.allclose(cols.nu[k + 6:], n1 - 1, rtol=1e-12)
    assert tc.columns(oracle, 1, 9, "benign").nan.all()         # n1 = 1: nu is 0 / 0


def test_separated_columns_set_the_risk_and_benign_ones_do_not(oracle):
    """wt_ttest_stat's `risk` (var * 1024 < meanSq in a set) by the columns' closed form: var = A^2 (n - odd) / n, meanSq = var + d^2 / 4."""
    for n1, n2 in tc.DELTA_SIZES:
        for family in ("benign", "separated"):
            cols = tc.columns(oracle, n1, n2, family)
            risk = np.zeros(len(cols), bool)
            for n, A in ((n1, cols.A1), (n2, cols.A2)):
                var = A * A * (n - n % 2) / n
                risk |= var * 1024.0 < var + cols.d * cols.d / 4
            if family == "benign":
                assert not risk.any(), (n1, n2)
            else:
                assert risk[(cols.A1 != 0) | (cols.A2 != 0) | (cols.d != 0)].all(), (n1, n2)


@pytest.mark.parametrize("size", tc.DELTA_SIZES, ids=_ids(tc.DELTA_SIZES))
def test_emulator_takes_the_difference_array_kernel_unpatched(oracle, size):
    """Every benign float set of >= 8 tracks: delta == 1, nothing patched or redone, and bit for bit the oracle (the emulator's tail
    is the oracle's form); the oracle's NaN positions are the reference's."""
    from emu import emu
    n1, n2 = size
    cols = tc.columns(oracle, n1, n2, "benign")
    t = cols.runlists()
    got, info = emu.reduce(t, "ttest", n_set0=n1)
    assert info["delta"] == 1 and info["W"] == 2048 and info["delta_bad"] == 0 and info["delta_redo"] == 0 and info["patched"] == 0, info
    exp = oracle.reduce(t.as_dict(), "ttest", n_set0=n1)
    assert_runs_equal(got, exp, 0.0, "benign %d v %d" % size)
    assert np.array_equal(exp[1], tc.positions_packed(len(cols))) and np.array_equal(np.isnan(exp[3]), cols.nan)


@pytest.mark.parametrize("size", [(8, 8), (50, 50), (1, 9)], ids=_ids([(8, 8), (50, 50), (1, 9)]))
def test_emulator_patches_or_redoes_the_separated_columns(oracle, size):
    """The layouts of the GPU cases below through the emulator's planner: separated columns in one window of seven are patched, in every
    window the launch is redone; NaN exactly where the reference has it."""
    from emu import emu
    n1, n2 = size
    if n1 > 1:
        t, parts = _patched_layout(oracle, n1, n2)
        got, info = emu.reduce(t, "ttest", n_set0=n1)
        assert info["delta"] == 1 and info["n_windows"] >= 6 and info["delta_bad"] == 1 and info["patched"] == 1, info
        assert_runs_equal(got, oracle.reduce(t.as_dict(), "ttest", n_set0=n1), 0.0, "patched %d v %d" % size)
        for cols, idx in parts:
            assert np.array_equal(np.isnan(got[3][idx]), cols.nan)
    cols, t, idx = _redone_layout(oracle, n1, n2)
    got, info = emu.reduce(t, "ttest", n_set0=n1)
    assert info["delta"] == 0 and info["delta_bad"] > 0 and info["patched"] == 0, info
    assert_runs_equal(got, oracle.reduce(t.as_dict(), "ttest", n_set0=n1), 0.0, "redone %d v %d" % size)
    assert np.array_equal(np.isnan(got[3][idx]), cols.nan)


def test_emulator_plans_chunks_for_2100_v_2100_float64(oracle):
    """4200 float64 tracks do not fit one workgroup's LDS: the general kernel runs the chunked plan (a few columns suffice to plan)."""
    from emu import emu
    cols = tc.columns(oracle, 2100, 2100, "benign")
    t = tc.columns_to_runlists(cols.M[:3], dtype=np.float64)
    got, info = emu.reduce(t, "ttest", n_set0=2100)
    assert info["delta"] == 0 and info["n_chunks"] > 1, info
    assert_runs_equal(got, oracle.reduce(t.as_dict(), "ttest", n_set0=2100), 0.0, "chunked")


# ---------------------------------------------------------------------------------------------------------------------------
# layouts shared by the emulator's and the device's cases
# ---------------------------------------------------------------------------------------------------------------------------
def _layout(parts):
    """parts: [(cols, positions)] -> RunLists (float32), [(cols, index of each of its columns in the output runs)]."""
    M = np.vstack([c.M for c, _ in parts])
    pos = np.concatenate([p for _, p in parts])
    rank = np.empty(len(pos), np.int64)
    rank[np.argsort(pos, kind="stable")] = np.arange(len(pos))
    out, k = [], 0
    for c, p in parts:
        out.append((c, rank[k:k + len(p)]))
        k += len(p)
    return tc.columns_to_runlists(M, pos), out


def _patched_layout(oracle, n1, n2):
    """Benign columns over six windows of 2048 bp, the separated ones (and the edge columns) all in a seventh between them:
    n_bad * 4 <= n_windows, so that window is patched."""
    ben, sep = tc.columns(oracle, n1, n2, "benign"), tc.columns(oracle, n1, n2, "separated")
    return _layout([(ben, tc.positions_spread(len(ben), [0, 1, 2, 4, 5, 6])), (sep, tc.positions_spread(len(sep), [3]))])


def _redone_layout(oracle, n1, n2):
    """Risky columns in every one of six windows: the general kernel redoes the launch.  (n1 = 1: var1 = 0 in every column.)"""
    cols = tc.columns(oracle, n1, n2, "separated" if n1 > 1 else "benign", None if n1 > 1 else 24)
    t, parts = _layout([(cols, tc.positions_spread(len(cols), [0, 1, 2, 3, 4, 5]))])
    return cols, t, parts[0][1]


def _coordinates(got, t, what):
    pos = np.unique(t.start)
    assert len(got[0]) == len(pos) and np.array_equal(got[1], pos) and np.array_equal(got[2], pos + 1) and not got[0].any(), what


def _same_bits(a, b, what):
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True), what


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    import torch
    assert torch.cuda.is_available()
    from wiggletools_amd import engine as E
    return E


def _run(engine, t, n1, flags=0):
    ts = engine.TrackSet.from_runlists(t)
    try:
        got = ts.reduce_host("ttest", flags=flags, n_set0=n1)
        return got, ts.stats()
    finally:
        ts.close()


@pytest.mark.gpu
@pytest.mark.parametrize("size", tc.DEVICE_SIZES, ids=_ids(tc.DEVICE_SIZES))
def test_gpu_benign_columns_on_every_kernel(oracle, engine, monkeypatch, size):
    """The benign columns of one pair of set sizes: as float tracks (the difference-array kernel from 8 tracks up, nothing patched; the
    general kernel below), as float64 tracks (the general kernel; 2100 v 2100: its chunked plan), 50 v 50 again with the difference
    arrays switched off, 16 v 17 and 450 v 450 under the other three strictness flags (every track is present everywhere: other code,
    same answer).  All within the bound of the true value and the same bit for bit."""
    n1, n2 = size
    cols = tc.columns(oracle, n1, n2, "benign")
    what = "%d v %d" % size
    t32 = cols.runlists()
    a, st = _run(engine, t32, n1)
    _coordinates(a, t32, what)
    if n1 + n2 >= 8:
        assert st["kernel"] == 1 and st["window_bp"] == 2048 and st["patched_windows"] == 0, st
        _hold(cols, a[3], "delta", what)
    else:
        assert st["kernel"] == 0, st
        _hold(cols, a[3], "general-few", what)
    b, st = _run(engine, cols.runlists(dtype=np.float64), n1)
    assert st["kernel"] == 0, st
    _hold(cols, b[3], "general-f64", what)
    _same_bits(a, b, what + ": float v float64 tracks")
    if size == (50, 50):
        monkeypatch.setenv("WTAMD_NO_DELTA_TTEST", "1")
        c, st = _run(engine, t32, n1)
        monkeypatch.delenv("WTAMD_NO_DELTA_TTEST")
        assert st["kernel"] == 0, st
        _hold(cols, c[3], "general-no-delta", what)
        _same_bits(a, c, what + ": difference arrays v general kernel")
    if size in ((16, 17), (450, 450)):
        for flags in (1, 2, 3):
            c, st = _run(engine, t32, n1, flags)
            assert st["kernel"] == 1 and st["patched_windows"] == 0, st
            _hold(cols, c[3], "delta-strict", what)
            _same_bits(a, c, what + ": flags %d" % flags)


PATCHED = [(8, 8), (16, 17), (50, 50), (33, 300)]


@pytest.mark.gpu
@pytest.mark.parametrize("size", PATCHED, ids=_ids(PATCHED))
def test_gpu_separated_columns_through_the_patch_kernel(oracle, engine, size):
    """Seven windows, the separated and the edge columns all in one: that window's values come from wt_patch_kernel -- the x side and the
    deep tail (and the reference's NaN) by wt_eval_finish<TTEST>; the float64 tracks' general kernel gives the same bits."""
    n1, n2 = size
    what = "patched %d v %d" % size
    t, parts = _patched_layout(oracle, n1, n2)
    ts = engine.TrackSet.from_runlists(t)
    a = ts.reduce_host("ttest", n_set0=n1)
    st = ts.stats()
    again = ts.reduce_host("ttest", n_set0=n1)      # the verdict is known: difference arrays and patch back to back
    st2 = ts.stats()
    ts.close()
    assert st["kernel"] == 1 and st["n_windows"] >= 6 and st["patched_windows"] == 1, st
    assert st2["kernel"] == 1 and st2["patched_windows"] == 1, st2
    _coordinates(a, t, what)
    for (cols, idx), route in zip(parts, ("delta", "patched")):
        _hold(cols, a[3][idx], route, what)
    _same_bits(a, again, what + ": second launch")
    t.value = t.value.astype(np.float64)
    b, st = _run(engine, t, n1)
    assert st["kernel"] == 0, st
    _same_bits(a, b, what + ": float v float64 tracks")


REDONE = [(8, 8), (50, 50), (2100, 2100)]


@pytest.mark.gpu
@pytest.mark.parametrize("size", REDONE, ids=_ids(REDONE))
def test_gpu_separated_columns_through_a_redone_launch(oracle, engine, size):
    """Risky columns in every window: the general kernel redoes the launch (`kernel == 0` after the verdict)."""
    n1, n2 = size
    what = "redone %d v %d" % size
    cols, t, idx = _redone_layout(oracle, n1, n2)
    a, st = _run(engine, t, n1)
    assert st["kernel"] == 0 and st["patched_windows"] == 0, st
    _coordinates(a, t, what)
    _hold(cols, a[3][idx], "redone", what)
    t.value = t.value.astype(np.float64)
    b, st = _run(engine, t, n1)
    assert st["kernel"] == 0, st
    _hold(cols, b[3][idx], "general-f64", what)
    _same_bits(a, b, what + ": float v float64 tracks")


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(2, 2), (2, 3), (1, 9)], ids=_ids([(2, 2), (2, 3), (1, 9)]))
def test_gpu_sets_under_three_tracks_are_refused(oracle, engine, size):
    """The reference's precondition (setComparisons.c:123-128), with its message: these columns' (t, nu) -- nu < 2, nu = 0 / 0 --
    reach the host-compiled tail above and never the device's."""
    from wiggletools_amd._lib import WtamdError
    cols = tc.columns(oracle, size[0], size[1], "benign", 24)
    for dtype in (np.float32, np.float64):
        ts = engine.TrackSet.from_runlists(cols.runlists(dtype=dtype))
        with pytest.raises(WtamdError, match="two sets with enough elements"):
            ts.reduce_host("ttest", n_set0=size[0])
        ts.close()


def _pipeline_layout(oracle, case, n1, n2):
    if case == "patched":
        return _patched_layout(oracle, n1, n2)
    ben = tc.columns(oracle, n1, n2, "benign")
    return _layout([(ben, tc.positions_spread(len(ben), [0, 1, 2, 3, 4, 5, 6]))])


@pytest.mark.parametrize("case", ["benign", "patched"])
def test_emulated_pipeline_on_the_columns(oracle, case):
    """The layouts of the next test through the emulated pipeline: batches of 3000 bp cut the windows elsewhere; the oracle's bits."""
    from emu import build as emu_build
    from wiggletools_amd.pipe import stream_runlists
    t, parts = _pipeline_layout(oracle, case, 16, 17)
    got, st = stream_runlists(t, "ttest", 3000, n_set0=16, lib=C.CDLL(emu_build.build_dropin()))
    assert st["batches"] >= 4, st
    assert_runs_equal(got, oracle.reduce(t.as_dict(), "ttest", n_set0=16), 0.0, case)
    for cols, idx in parts:
        assert np.array_equal(np.isnan(got[3][idx]), cols.nan)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["benign", "patched"])
def test_gpu_columns_through_the_pipeline(oracle, engine, case):
    """The streaming pipeline (wtamd_pipe_*) in batches of 3000 bp: the same columns, the same bound, the track set's bits."""
    from wiggletools_amd.pipe import stream_runlists
    n1, n2 = 16, 17
    t, parts = _pipeline_layout(oracle, case, n1, n2)
    got, st = stream_runlists(t, "ttest", 3000, n_set0=n1, lib=None)
    assert st["batches"] >= 4 and st["delta_batches"] >= 1, st
    _coordinates(got, t, case)
    for cols, idx in parts:
        _hold(cols, got[3][idx], "pipe", "%s %d v %d" % (case, n1, n2))
    direct, _ = _run(engine, t, n1)
    _same_bits(got, direct, case + ": pipeline v track set")
