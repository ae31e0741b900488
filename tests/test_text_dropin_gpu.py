"""wtamd_TeeWiggleIterator and wtamd_toFile of the product over array children, an overlapping child, popping children and
reducers of this library, with the device door and again with WTAMD_NO_DEVICE_TEXT=1: the file byte for byte the reference's
(tests/text_dropin.py, which tests/test_text_dropin_host.py runs over the emulated drop-in library); a reducer's file against
the all-reference harness's `write` / `write_bg` of the same reducer, as tests/test_mixed_link.py compares the reference's
writer."""
import os

import numpy as np
import pytest

import text_dropin
import text_model as M
from helpers import random_case

pytestmark = pytest.mark.gpu

_KEEP = []


@pytest.fixture(scope="module", autouse=True)
def _pools_as_a_fresh_process_has_them():
    """The staging buffers of these tests rest in the library's process-wide pools afterwards; tests that count the pools'
    misses (tests/test_trackset_pool.py) expect to meet nothing larger than their own buffers there."""
    yield
    from wiggletools_amd import _lib
    _lib.lib().wtamd_pool_trim()


def test_dropin(tmp_path):
    from wiggletools_amd import _lib
    _lib.lib()                                  # (PyTorch's HIP runtime goes first, whichever test file runs first: _lib.py)

    def setenv(k, v):
        os.environ[k] = v

    try:
        text_dropin.check_dropin(text_dropin.DropIn(_lib.LIB_PATH), tmp_path, setenv)
    finally:
        os.environ.pop("WTAMD_NO_DEVICE_TEXT", None)


def _readers(t):
    from wiggletools_amd import dropin
    kids = []
    for i in range(t.n_tracks):
        seg, S, F, V = [0], [], [], []
        for c in range(t.n_chrom):
            a, b = t.seg_off[c * t.n_tracks + i], t.seg_off[c * t.n_tracks + i + 1]
            S.append(t.start[a:b]); F.append(t.finish[a:b]); V.append(t.value[a:b])
            seg.append(seg[-1] + int(b - a))
        s, f, v = (np.ascontiguousarray(np.concatenate(x), dt) for x, dt in ((S, np.int32), (F, np.int32), (V, np.float32)))
        _KEEP.append((s, f, v))
        kids.append(dropin.array_reader(list(t.chrom_names), seg, s.ctypes.data, f.ctypes.data, v.ctypes.data, float(t.defaults[i])))
    return kids


def _flat_tracks():
    """Two tracks of touching runs with one value per long stretch: the mean's runs merge into groups of thousands of runs,
    which small batches cut many times."""
    from wiggletools_amd.runlists import RunLists
    tracks = []
    for t in range(2):
        chroms = []
        for c in range(2):
            w = 7 + 3 * t
            chroms.append([(1 + k * w, 1 + (k + 1) * w, float(1 + (k * w) // 9000)) for k in range(3000)])
        tracks.append(chroms)
    return RunLists.from_lists(tracks, dtype=np.float32)


@pytest.mark.parametrize("small_batches", [False, True])
def test_a_reducer_of_this_library_against_the_reference_writer(oracle, tmp_path, monkeypatch, small_batches):
    """A group of the compression rule spans many batches when the batches are a few hundred base pairs."""
    from wiggletools_amd import dropin
    if not oracle.have_ref():
        pytest.skip("compiled reference not available")
    R = oracle.ref_harness()
    if small_batches:
        monkeypatch.setenv("WTAMD_MIN_SPAN", "700")
        monkeypatch.setenv("WTAMD_BATCH_INTERVALS", "256")
    for t in (random_case(9700, max_len=4000, dtype=np.float32), _flat_tracks()):
        d = t.as_dict()
        for op in ("mean", "max"):
            for bg in (False, True):
                dropin.to_file(dropin.reducer(op, _readers(t)), tmp_path / "a.txt", bedgraph=bg)
                a = open(tmp_path / "a.txt").read()
                b = R.write_reduce(d, op, tmp_path / "b.txt", bedgraph=bg)
                assert a == b, (op, bg, len(a), len(b))
                assert len(b) > 0


def test_python_dropin_tee(tmp_path):
    from wiggletools_amd import dropin
    L = M.mergeable_list()
    s, f, v = L.s, L.f, np.ascontiguousarray(L.v, np.float32)
    kid = dropin.array_reader([n.decode() for n in L.names], L.seg, s.ctypes.data, f.ctypes.data, v.ctypes.data)
    wi, close = dropin.tee_iterator(kid, tmp_path / "t.wig")
    n = dropin.drain_pops(wi)[0]
    close()
    C = M.compress(L)
    assert n == len(C) < len(L) and open(tmp_path / "t.wig", "rb").read() == M.text(C, 0)[0]
