"""Are the kernels' barriers enough?  The emulator (tests/emu/wt_emu.cpp) runs one loop over the lanes per __syncthreads() interval
of the kernel it restates, wave by wave, and the order of the waves inside an interval is a parameter: on the device it is arbitrary,
so whatever the order, the output has to be the same bit for bit.  `forward` (what every other emulator test runs) is held to the
oracle at the tolerance tests/test_emu_parity.py uses for the op; `reverse`, `rotate:1` and two `shuffle` seeds are held to `forward`
exactly.  The cases sit where intervals are shared and LDS regions are reused: dense windows of the difference-array kernels (the
staging reuses the accumulators), chunked tracks, redone and patched windows, one- and two-wave workgroups, the general kernel in
every flavour, the walking kernels' plain phases."""
import numpy as np
import pytest

from helpers import ALL_MULTIPLEX_OPS, assert_runs_equal, random_case
from emu import emu
from wiggletools_amd.runlists import RunLists, synth

ORDERS = ["reverse", "rotate:1", "shuffle:1", "shuffle:2"]
GEOMS = [(None, None), (4, 64), (1, 64), (4, 128), (1, 128)]   # as tests/test_emu_parity.py
# tolerance against the oracle, as tests/test_emu_parity.py: bit for bit, but 1e-12 for the var family
TOL = {"var": 1e-12, "stddev": 1e-12, "cv": 1e-12}


def _all_orders(t, op, what, exp=None, tol=0.0, **kw):
    """forward against the oracle (exp), every other order against forward bit for bit; returns forward's output and info."""
    fwd, info = emu.reduce(t, op, wave_order="forward", **kw)
    if exp is not None:
        if len(fwd) == 5:
            assert len(fwd[0]) == len(exp[0]), what
            for a, b in zip(fwd, exp):
                assert np.array_equal(a, b, equal_nan=True), what
        else:
            assert_runs_equal(fwd, exp, tol, "%s, forward vs oracle" % what)
    names = ("chrom", "start", "finish", "value") if len(fwd) == 4 else ("chrom", "start", "finish", "tile", "inplay")
    for order in ORDERS:
        got, info2 = emu.reduce(t, op, wave_order=order, **kw)
        assert info2 == info, "%s, %s: %s != %s" % (what, order, info2, info)
        assert len(got[0]) == len(fwd[0]), "%s, %s: %d runs, forward %d" % (what, order, len(got[0]), len(fwd[0]))
        for name, a, b in zip(names, got, fwd):
            if not np.array_equal(a, b, equal_nan=True):
                same = (a == b) | ((a != a) & (b != b))
                bad = np.flatnonzero(~same.reshape(len(a), -1).all(axis=1))
                raise AssertionError("%s: wave order %s changes %d of %d %ss; the runs starting at %s ... (%s)"
                                     % (what, order, len(bad), len(a), name, fwd[1][bad[:8]].tolist(), info))
    return fwd, info


# ---- difference-array kernel (wt_delta_kernel) ----
def _dense(n_bp, mean_run, n_tracks=100, seed=3):
    return synth(n_tracks, [n_bp], mean_run=mean_run, seed=seed, gap_prob=0.0, dtype=np.float32, value_levels=800)


@pytest.mark.parametrize("mean_run", [1.0, 16.0])
@pytest.mark.parametrize("op", ["sum", "mean", "mean_df", "var", "stddev", "cv", "max", "min"])
def test_wave_order_delta_dense_windows(oracle, op, mean_run):
    """Every family of wt_delta_kernel on more than five windows of its own width, 100 tracks, a breakpoint at (nearly) every position:
    the staged runs fill acc[] / ev[] to the top."""
    W = {"var": 4096, "stddev": 4096, "cv": 4096}.get(op, 8192)
    t = _dense(5 * W + W // 2, mean_run)
    if op == "mean_df":         # non-zero defaults: wt_delta_kernel<mean, DF>
        t = RunLists(t.n_chrom, t.n_tracks, t.seg_off, t.start, t.finish, t.value, np.where(np.arange(t.n_tracks) % 3 == 0, 1.5, 0.0))
        op = "mean"
    fwd, info = _all_orders(t, op, "%s mean run %g" % (op, mean_run), oracle.reduce(t.as_dict(), op), TOL.get(op, 0.0))
    assert info["delta"] == 1 and info["delta_bad"] == 0 and info["W"] == W and info["n_windows"] >= 6, info


@pytest.mark.parametrize("mean_run", [1.0, 16.0])
def test_wave_order_delta_ttest_dense_windows(oracle, mean_run):
    """wt_delta_kernel<ttest>: 2048-bp windows, 768 lanes, 50 v 50.  With the spare entries of WT_STAGE_AT (r + r / 32) the emitted run
    number 1986 and later of a window is staged at acc[W ..], where the p-values of the window's first positions lie until their own
    lanes (wave 0) have loaded them: asserted from the output that windows that dense are there.  (Before the barrier between
    wt_delta_load_res_tt and the staging: `wave order reverse changes 310 of 12000 values; the runs starting at [1, 2, 3, 4, 5, 6, 7,
    8] ...` -- the runs starting at positions 1 ... 62 of each full window -- and 300 of 11988 at mean run 16.)"""
    t = _dense(12000, mean_run)
    exp = oracle.reduce(t.as_dict(), "ttest", n_set0=50)
    per_window = np.bincount(exp[1] // 2048)
    assert per_window.max() >= 1987 and (per_window >= 1987).sum() >= 5, per_window     # the precondition of the race
    fwd, info = _all_orders(t, "ttest", "ttest mean run %g" % mean_run, exp, 0.0, n_set0=50)     # (k/8 values: bit for bit)
    assert info["delta"] == 1 and info["delta_bad"] == 0 and info["W"] == 2048 and info["T"] == 768, info


def test_wave_order_delta_ttest_full_mantissas_and_strict_flags(oracle):
    """Full mantissas (1e-9 against the oracle, as tests/test_emu_parity.py::test_emu_delta_ttest), the four strictness flags."""
    rng = np.random.default_rng(5)
    t = _dense(7000, 3.0, n_tracks=40, seed=9)
    t.value[:] = (t.value * rng.choice([0.3, 1.0], len(t.value))).astype(np.float32)
    for flags in (0, 1, 2, 3):
        fwd, info = _all_orders(t, "ttest", "ttest flags %d" % flags, oracle.reduce(t.as_dict(), "ttest", flags=flags, n_set0=17), 1e-9,
                                flags=flags, n_set0=17)
        assert info["delta"] == 1, info


def test_wave_order_delta_more_tracks_than_lanes(oracle):
    """1100 tracks on 1024 (768) lanes: the track ranges are rebuilt per chunk between the passes (nchunks > 1)."""
    t = synth(1100, [17000], mean_run=40.0, seed=4, gap_prob=0.1, dtype=np.float32, value_levels=800)
    for op in ("mean", "var", "max"):
        fwd, info = _all_orders(t, op, "1100 tracks %s" % op, oracle.reduce(t.as_dict(), op), TOL.get(op, 0.0))
        assert info["delta"] == 1 and info["T"] < 1100, info


@pytest.mark.parametrize("direction", ["falling", "rising"])
def test_wave_order_delta_redone_windows(oracle, direction):
    """The speculative unit does not fit a window: accumulators cleared and the pass repeated (wt_delta_rezero between two barriers)."""
    t = synth(7, [30000], mean_run=6.0, seed=21, gap_prob=0.1, dtype=np.float32)
    t.value[:] = (np.random.default_rng(22).random(len(t.value)) + 1.0).astype(np.float32)
    step = 3 if direction == "rising" else -3
    t.value[:] = np.ldexp(t.value.astype(np.float64), step * (t.start.astype(np.int64) // 2048)).astype(np.float32)
    for op in ("sum", "mean"):
        fwd, info = _all_orders(t, op, "redo %s %s" % (direction, op), oracle.reduce(t.as_dict(), op), 0.0, delta_T=256)
        assert info["delta"] == 1 and info["delta_bad"] == 0 and info["delta_redo"] > 0 and info["T"] == 256, info


@pytest.mark.parametrize("kind", ["wide", "nan"])
def test_wave_order_delta_patched_windows(oracle, kind):
    """A window the difference arrays cannot prove exact keeps its runs and gets its values from wt_patch_kernel: four 512-bp windows
    of 128 lanes under each 2048-bp window of 256."""
    t = synth(12, [30000, 300], mean_run=8.0, seed=5, gap_prob=0.1, dtype=np.float32)
    t.value[:] = (np.random.default_rng(6).random(len(t.value)) + 0.5).astype(np.float32)
    if kind == "wide":
        t.value[3] = np.float32(1e-30)
    else:
        t.value[7] = np.nan
        t.value[len(t.value) // 2] = np.nan
    for op in ("sum", "mean", "var") + (("max",) if kind == "nan" else ()):        # (a wide exponent range is nothing to Max)
        fwd, info = _all_orders(t, op, "patched %s %s" % (kind, op), oracle.reduce(t.as_dict(), op), TOL.get(op, 0.0), delta_T=256, ppt=4, T=128)
        assert info["delta"] == 1 and info["delta_bad"] > 0 and info["patched"] == info["delta_bad"], info


@pytest.mark.parametrize("T", [64, 128])
def test_wave_order_delta_one_and_two_waves(oracle, T):
    """One wave: every order is `forward`; two: rotate:1 is reverse."""
    t = synth(9, [5000, 700], mean_run=3.0, seed=31, gap_prob=0.1, dtype=np.float32, value_levels=800)
    for op in ("sum", "mean", "var", "min"):
        fwd, info = _all_orders(t, op, "T %d %s" % (T, op), oracle.reduce(t.as_dict(), op), TOL.get(op, 0.0), delta_T=T)
        assert info["delta"] == 1 and info["T"] == T and info["W"] == 8 * T, info


def test_wave_order_delta_sparse_windows(oracle):
    t = synth(100, [60000], mean_run=3000.0, seed=8, gap_prob=0.05, dtype=np.float32, value_levels=800)
    for op, kw in (("sum", {}), ("mean", {}), ("var", {}), ("max", {}), ("ttest", dict(n_set0=50))):
        fwd, info = _all_orders(t, op, "sparse %s" % op, oracle.reduce(t.as_dict(), op, **kw), TOL.get(op, 0.0), **kw)
        assert info["delta"] == 1, info


# ---- general kernel (wt_reduce_kernel) ----
@pytest.mark.parametrize("seed", range(10))
def test_wave_order_general_kernel(oracle, seed):
    """Every op of the bitmap kernel, the two-sample ops under the four strictness flags and the multiplexer tile, all-resident tracks
    and chunked ones (MULTI), over the geometries of tests/test_emu_parity.py (None: the plan's own, several waves)."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(6, 13))
    t = random_case(4000 + seed, n_tracks=n, max_len=1500, dtype=np.float64 if seed % 2 else np.float32)
    d = t.as_dict()
    ppt, T = GEOMS[seed % len(GEOMS)]
    n1 = int(rng.integers(3, n - 2))
    for chunk in (None, int(rng.integers(1, n))):
        kw = dict(ppt=ppt, T=T, chunk=chunk)
        for op in ALL_MULTIPLEX_OPS:
            _all_orders(t, op, "seed %d %s chunk %s" % (seed, op, chunk), oracle.reduce(d, op, flags=seed & 1), 0.0, flags=seed & 1, **kw)
        _all_orders(t, "sum", "seed %d tile chunk %s" % (seed, chunk), oracle.multiplex(d, flags=seed & 1), flags=seed & 1, multiplex=True, **kw)
        for flags in (0, 1, 2, 3):
            for op in ("ttest", "mwu"):
                _all_orders(t, op, "seed %d %s flags %d chunk %s" % (seed, op, flags, chunk), oracle.reduce(d, op, flags=flags, n_set0=n1),
                            1e-12 if op == "ttest" else 0.0, flags=flags, n_set0=n1, **kw)


@pytest.mark.parametrize("seed", range(3))
def test_wave_order_general_kernel_global_scratch(oracle, seed):
    rng = np.random.default_rng(50 + seed)
    n = int(rng.integers(6, 13))
    t = random_case(4100 + seed, n_tracks=n, max_len=1500, dtype=np.float64 if seed % 2 else np.float32)
    d = t.as_dict()
    chunk = int(rng.integers(1, n + 1)) if seed else None
    n1 = int(rng.integers(2, n - 1))
    fwd, info = _all_orders(t, "median", "median", oracle.reduce(d, "median"), 0.0, chunk=chunk, global_scratch=1)
    assert info["scratch_slab"] > 0
    for flags in (0, 1, 2, 3):
        fwd, info = _all_orders(t, "mwu", "mwu flags %d" % flags, oracle.reduce(d, "mwu", flags=flags, n_set0=n1), 0.0, flags=flags, n_set0=n1,
                                chunk=chunk, global_scratch=1)
        assert info["scratch_slab"] > 0


# ---- walking kernels (wt_walk_kernel, wt_mwalk_kernel): the plain phases; the stretch-walking rounds stay as they are ----
@pytest.mark.parametrize("pair", [0, 1])
@pytest.mark.parametrize("ov", [None, 0])
def test_wave_order_median_walk(oracle, pair, ov):
    t = synth(33, [5000, 300], mean_run=5.0, seed=12 + pair, gap_prob=0.05, dtype=np.float32, value_levels=5, nan_prob=0.002)
    fwd, info = _all_orders(t, "median", "median walk pair %d ov %s" % (pair, ov), oracle.reduce(t.as_dict(), "median"), 0.0,
                            walk_T=256, walk_S=8, walk_capp=2, walk_ov=ov, walk_pair=pair)
    assert info["walk"] == 1 and info["T"] >= 128 and (ov is None or info["walk_fallback"] > 0), info


@pytest.mark.parametrize("ov", [None, 0])
def test_wave_order_mwu_walk(oracle, ov):
    t = synth(50, [2500, 300], mean_run=5.0, seed=17, gap_prob=0.05, dtype=np.float32, value_levels=25)
    for flags in (0, 3):
        fwd, info = _all_orders(t, "mwu", "mwu walk ov %s flags %d" % (ov, flags), oracle.reduce(t.as_dict(), "mwu", flags=flags, n_set0=20), 0.0,
                                flags=flags, n_set0=20, walk_S=8, walk_capp=2, walk_ov=ov, mwalk=1)
        assert info["walk"] == 1 and info["T"] >= 128 and (ov is None or info["walk_fallback"] > 0), info
