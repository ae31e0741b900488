"""Multi-column wig, bedGraph and paste text on the device (csrc/wt_mtext.hip: wtamd_tile_text, wtamd_trackset_mtext) against the
Python model of tests/mtext_model.py.  No tolerance exists here: every byte is equal."""
import numpy as np
import pytest

import mtext_model as M

pytestmark = pytest.mark.gpu

CASES = M.cases()


@pytest.fixture(scope="module", autouse=True)
def _pools_as_a_fresh_process_has_them():
    """The staging buffers of these tests rest in the library's process-wide pools afterwards; tests that count the pools'
    misses (tests/test_trackset_pool.py) expect to meet nothing larger than their own buffers there."""
    yield
    from wiggletools_amd import _lib
    _lib.lib().wtamd_pool_trim()


def _door(T, flags=0, state=None, capacity=None, offset=0, width=None, prefix_mode="both", host=False, **_):
    from wiggletools_amd import engine
    if capacity is None:
        capacity = len(M.text(T, flags, state)[0])
    return engine._mtext_door(T.L.names, T.L.seg, T.L.s, T.L.f, T.vals, T.prefixes, flags, state, capacity, offset, width, prefix_mode, host)


def _host_door(T, **kw):
    return _door(T, host=True, **kw)


@pytest.fixture(scope="module")
def device_texts():
    """Every case in its modes through the door, once: {(name, flags): bytes} (the state and the canaries checked on the way)."""
    return {(name, flags): M.check_case(_door, name, flags) for name, T in CASES.items() for flags in M.flags_of(T)}


def test_every_width_and_count_is_the_model_text(device_texts):
    """Widths 1, 2, 3, 63, 64, 65, 257 with 1, 255, 256, 257 entries, and 9999 .. 20001 entries at width 3; rows of 2048 cells,
    longer than the window, one to five copies of them; every special value in every column of width 5 and cells at the edge
    of 2^64; point-by-point runs across entry 10000, a chromosome change, start > the last finish; prefixes of 0, 1, 15, 16,
    17 and 20000 bytes."""
    for w in M.SMALL_WIDTHS:
        for n in M.SMALL_COUNTS:
            assert ("w%d_n%d" % (w, n), 0) in device_texts and CASES["w%d_n%d" % (w, n)].vals.shape == (n, w)
    for n in M.BIG_COUNTS:
        assert ("w3_n%d" % n, M.BEDGRAPH) in device_texts
    for name in ("w2048_n40", "specials_w5", "points_across_10000_w2", "straddle_10000_w2", "chrom_change_w2", "transitions_gaps_w3", "paste_w3"):
        assert (name, 0) in device_texts
    assert {len(p) for p in CASES["paste_w3"].prefixes} >= set(M.PREFIX_LENGTHS)
    assert 2.0 ** 64 - 2048.0 in CASES["specials_w5"].vals


@pytest.mark.parametrize("name", ["w3_n20001", "straddle_10000_w2", "points_across_10000_w2", "chrom_change_w2", "paste_w1_n10001"])
def test_cut_tiles_chain_through_the_state(name):
    for flags in M.flags_of(CASES[name]):
        M.check_chained(_door, name, flags)


def test_the_same_bytes_on_a_second_call(device_texts):
    for name in ("w3_n20001", "w2048_n40", "paste_w3"):
        assert M.check_case(_door, name, 0) == device_texts[(name, 0)]


@pytest.mark.parametrize("name", ["w3_n257", "w65_n256", "paste_w3"])
def test_any_alignment_and_the_exact_capacity(name):
    """text at byte offsets 0 .. 15 of an allocation with the canaries on both sides intact; capacity - 1 is refused with the
    size needed and not one byte written."""
    for flags in M.flags_of(CASES[name]):
        M.check_alignment_and_capacity(_door, name, flags)


def test_refusals_and_wide_cells_write_nothing():
    M.check_refusals(_door)


def test_an_empty_call_leaves_the_state_alone():
    st = {"in_block": 17, "point_by_point": 1, "last_finish": 99, "continues": 0}
    rc, buf, nb, nw, st2 = _door(CASES["w3_n257"].part(0, 0), 0, state=st, capacity=0, width=3)
    assert (rc, nb, nw, st2) == (0, 0, 0, st) and (buf == M.CANARY).all()


def test_the_host_door_equals_the_device_door(device_texts):
    for name in ("w3_n10001", "w257_n257", "paste_w3", "chrom_change_w2"):
        assert M.check_case(_host_door, name, 0) == device_texts[(name, 0)]
    M.check_refusals(_host_door)


def _trackset():
    from wiggletools_amd import runlists
    rl = runlists.synth(5, [3000, 2500, 1800], mean_run=3, gap_prob=0.3, seed=77, dtype=np.float64, defaults=[0.0, 1.5, -2.0, 0.25, 7.0])
    rl.chrom_names = ["chr1", "chr2", "chrX"]
    return rl


@pytest.mark.parametrize("strict", [False, True])
def test_trackset_mtext_is_tile_text_of_the_multiplexed_tile(strict):
    from wiggletools_amd import engine
    rl = _trackset()
    ts = engine.TrackSet.from_runlists(rl)
    chrom, s, f, tile, _ = ts.multiplex_host(engine.STRICT_SET0 if strict else 0)
    assert len(s) > 300 and tile.shape[1] == 5
    seg = np.concatenate([[0], np.cumsum(np.bincount(chrom, minlength=3))])
    T = M.Tile(M.Lists(rl.chrom_names, seg, s, f, np.zeros(len(s))), tile)
    for bed in (False, True):
        expect = M.text(T, M.BEDGRAPH if bed else 0)[0]
        assert engine.tile_text(rl.chrom_names, seg, s, f, tile, bedgraph=bed) == expect
        got = ts.mtext(rl.chrom_names, bedgraph=bed, strict=strict)             # TrackSet.mtext returns the file
        assert got == expect, M.first_difference(got, expect)
    if not strict:
        assert (tile == 1.5).any() and b"\t7.000000\n" in expect                # defaults of tracks not in play are printed
    ts.close()
