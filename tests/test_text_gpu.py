"""Wig and bedGraph text on the device (csrc/wt_text.hip: wtamd_runs_text) against the Python model of tests/text_model.py, which
tests/golden/make_text_golden.py holds byte for byte to what the compiled reference's TeeWiggleIterator printed, and against the
recorded texts themselves (tests/golden/text_fixtures.json).  No tolerance exists here: every byte is equal."""
import numpy as np
import pytest

import text_model as M

pytestmark = pytest.mark.gpu

CASES = M.cases()


@pytest.fixture(scope="module", autouse=True)
def _pools_as_a_fresh_process_has_them():
    """The staging buffers of these tests rest in the library's process-wide pools afterwards; tests that count the pools'
    misses (tests/test_trackset_pool.py) expect to meet nothing larger than their own buffers there."""
    yield
    from wiggletools_amd import _lib
    _lib.lib().wtamd_pool_trim()


def _door(L, flags, state=None, capacity=None, offset=0, dtype=np.float64, names=None, seg=None, n_seg=None):
    from wiggletools_amd import engine
    from wiggletools_amd.runlists import RunLists
    rl = RunLists(len(L.names), 1, L.seg, L.s, L.f, L.v.astype(dtype), [0.0], [n.decode("latin-1") for n in L.names])
    return engine._text_door(rl, flags, state, capacity, offset, names, seg, n_seg)


@pytest.fixture(scope="module")
def device_texts():
    """Every case in both modes through the door, once: {fixture name: bytes} (the state and the canaries checked on the way)."""
    return {"%s/%d" % (name, flags): M.check_case(_door, L, flags, (name, flags)) for name, L in CASES.items() for flags in (0, M.BEDGRAPH)}


def test_fixtures_byte_for_byte(device_texts):
    """The transitions, chromosome changes, gaps and adjacency, the stretch across entry 10000, names of 1 and 255 bytes, the
    coordinates' ends and every special value: what the reference printed."""
    fx = [c for c in M.fixtures() if c["case"] in CASES]        # (the wide lists are the host sweep's: tests/test_text_emu.py)
    assert len(fx) == len(device_texts)
    for c in fx:
        M.check_against_fixture(c, CASES[c["case"]], c["flags"], device_texts[c["name"]])


def test_run_counts_around_a_tile_and_a_block(device_texts):
    for n in (1, 255, 256, 257, 9999, 10000, 10001, 20001):
        assert len(CASES["random_%d" % n]) == n and "random_%d/0" % n in device_texts


@pytest.mark.parametrize("name", ["random_20001", "straddle_10000", "points_across_10000", "chrom_change"])
def test_cut_lists_chain_through_the_state(name):
    for flags in (0, M.BEDGRAPH):
        M.check_chained(_door, CASES[name], flags, (name, flags))


def test_f32_equals_f64_of_the_widened_values():
    for name in ("values_f32", "random_10001"):
        L = CASES[name].as_f32()
        for flags in (0, M.BEDGRAPH):
            assert M.check_case(_door, L, flags, name, dtype=np.float32) == M.check_case(_door, L, flags, name, dtype=np.float64)


def test_the_same_bytes_on_a_second_call(device_texts):
    for name in ("random_20001", "values"):
        assert M.check_case(_door, CASES[name], 0, name) == device_texts[name + "/0"]


@pytest.mark.parametrize("name", ["random_257", "random_10001", "names"])
def test_any_alignment_and_the_exact_capacity(name):
    """text at byte offsets 0 .. 3 of an allocation with the canaries on both sides intact; capacity - 1 is refused with the
    size needed and not one byte written."""
    M.check_alignment_and_capacity(_door, CASES[name], 0, name)
    M.check_alignment_and_capacity(_door, CASES[name], M.BEDGRAPH, name)


def test_refusals_and_wide_values_write_nothing():
    M.check_refusals(_door)


def test_run_counts_and_offsets_the_door_refuses():
    """Fewer than 0 or at least 2^31 runs, offsets that decrease or do not start at 0, n_seg < 0: WTAMD_ERR_ARG before a run
    is looked at, nothing written, the state untouched."""
    M.check_count_refusals(_door)


def test_an_empty_call_leaves_the_state_alone():
    st = {"in_block": 17, "point_by_point": 1, "last_finish": 99, "continues": 0}
    rc, buf, nb, nw, st2 = _door(CASES["random_255"].part(0, 0), 0, state=st, capacity=0)
    assert (rc, nb, nw, st2) == (0, 0, 0, st) and (buf == M.CANARY).all()


def test_text_runlists_returns_the_file():
    from wiggletools_amd import engine
    from wiggletools_amd.runlists import RunLists
    L = CASES["chrom_change"]
    rl = RunLists(len(L.names), 1, L.seg, L.s, L.f, L.v, [0.0], [n.decode() for n in L.names])
    assert engine.text_runlists(rl) == M.text(L, 0)[0]
    assert engine.text_runlists(rl, bedgraph=True) == M.text(L, M.BEDGRAPH)[0]
    assert engine.TEXT_CANARY == M.CANARY
