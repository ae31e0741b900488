"""A fresh zero-copy track set on the library's pools (csrc/wt_pool.h): its device tables, counters, staging and extents
buffers come from the process-wide pools and return to them -- a second set of the same shape allocates nothing, a buffer
returns only after the device has finished with it, and what a set reads back (extents, window tables) is its own data.
All cases: 8 tracks x 2.4 Mbp at a mean run of 16 bp, about 300 windows of the difference-array kernel."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_TRACKS, LENGTH = 8, 2_400_000
_ref = {}


def _data(seed, lens=(LENGTH,), first_start=1):
    from wiggletools_amd.runlists import synth
    return synth(N_TRACKS, list(lens), mean_run=16, gap_prob=0.02, seed=seed, first_start=first_start)


def _expect(oracle, key, rl, op="mean"):
    """The oracle's runs of a data set, computed once per (data set, op)."""
    if (key, op) not in _ref:
        _ref[(key, op)] = oracle.reduce(rl.as_dict(), op)
    return _ref[(key, op)]


def _stats():
    from wiggletools_amd import _lib
    a = (C.c_int64 * 6)()
    _lib.lib().wtamd_pool_stats(a)
    return list(a)


def _to_device(rl):
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    return (torch.from_numpy(rl.start).to(dev), torch.from_numpy(rl.finish).to(dev), torch.from_numpy(rl.value).to(dev))


def _zero_copy(rl, tensors=None):
    from wiggletools_amd import engine
    s, f, v = tensors if tensors is not None else _to_device(rl)
    return engine.TrackSet.from_device(rl.n_chrom, rl.n_tracks, rl.seg_off, s, f, v, rl.defaults)


def _got(out, n_chrom):
    """(chrom, start, finish, value) of a DeviceRuns the device has finished writing; the run count is chrom_run_off's last entry."""
    cro = out.chrom_run_off.cpu().numpy()
    n = int(cro[-1])
    chrom = np.repeat(np.arange(n_chrom, dtype=np.int32), np.diff(cro))
    return chrom, out.start[:n].cpu().numpy(), out.finish[:n].cpu().numpy(), out.value[:n].cpu().numpy()


def _run(rl, op="mean", tensors=None):
    """create -> index -> reduce -> close of a zero-copy set; the runs and the library's statistics"""
    ts = _zero_copy(rl, tensors)
    ts.index(op)
    out = ts.alloc_runs()
    n = ts.reduce(op, out)
    st = ts.stats()
    got = _got(out, rl.n_chrom)
    assert len(got[0]) == n
    ts.close()
    return got, st


def test_second_set_of_the_same_shape_allocates_nothing(oracle):
    """(a) and (b): the second set leaves the pools' miss counters where they were; a set four times longer grows."""
    import torch
    from helpers import assert_runs_equal
    assert torch.cuda.is_available()
    a, b = _data(11), _data(12)
    got, st = _run(a)
    assert st["kernel"] == 1 and 250 <= st["n_windows"] <= 350, st
    assert_runs_equal(got, _expect(oracle, "a", a), 0.0, "first set")
    s1 = _stats()
    got, _ = _run(b)
    s2 = _stats()
    assert_runs_equal(got, _expect(oracle, "b", b), 0.0, "second set")
    for k in (0, 1, 3, 4):
        assert s2[k] == s1[k], (k, s1, s2)              # nothing page-locked, nothing mapped
    assert s2[2] > 0 and s2[5] > 0, s2                  # its buffers rest in the pools again
    long4 = _data(13, lens=(4 * LENGTH,))
    got, st = _run(long4)
    assert st["n_windows"] > 1000, st
    assert_runs_equal(got, _expect(oracle, "long4", long4), 0.0, "set four times longer")
    assert _stats()[3] > s2[3]                          # (its tables are larger than anything that rested: mapped afresh)


def _stretch(rl, factor, shift):
    """The same number of runs per segment at other coordinates: extents `factor` times larger, moved by `shift`."""
    from wiggletools_amd.runlists import RunLists
    s = (rl.start.astype(np.int64) - 1) * factor + 1 + shift
    f = (rl.finish.astype(np.int64) - 1) * factor + 1 + shift
    v = np.roll(rl.value, 7)
    return RunLists(rl.n_chrom, rl.n_tracks, rl.seg_off, s.astype(np.int32), f.astype(np.int32), v, rl.defaults)


@pytest.mark.parametrize("lens", [(LENGTH,), (LENGTH // 2, 0, LENGTH // 2)], ids=["one_chrom", "three_chroms_middle_empty"])
def test_rewritten_in_place_and_indexed_again(oracle, lens):
    """(c) and (c'): the tensors of a zero-copy set are overwritten with run lists of larger extents and another window count;
    `index` reads the extents again and rebuilds (and grows) the window tables."""
    import torch
    from helpers import assert_runs_equal
    key = "c%d" % len(lens)
    a = _data(21, lens=lens)
    b = _stretch(a, 3, 5000)
    tensors = _to_device(a)
    ts = _zero_copy(a, tensors)
    ts.index("mean")
    out = ts.alloc_runs(capacity=2 * int(a.seg_off[-1]))
    n = ts.reduce("mean", out)
    w_before = ts.stats()["n_windows"]
    got = _got(out, a.n_chrom)
    assert len(got[0]) == n
    assert_runs_equal(got, _expect(oracle, key + "/before", a), 0.0, "before the rewrite")
    for t, x in zip(tensors, (b.start, b.finish, b.value)):
        t.copy_(torch.from_numpy(x))
    ts.index("mean")
    n = ts.reduce("mean", out)
    st = ts.stats()
    got = _got(out, a.n_chrom)
    ts.close()
    assert len(got[0]) == n and st["n_windows"] > 2 * w_before, (w_before, st)
    assert_runs_equal(got, _expect(oracle, key + "/after", b), 0.0, "after the rewrite")


def test_close_with_a_launch_in_flight_then_reuse(oracle):
    """(d): reduce(sync=False) on a side stream and close() at once; a new set of OTHER data then takes the same buffers from
    the pool and reduces on the default stream.  Both outputs equal the oracle: close() waited for the device."""
    import torch
    from helpers import assert_runs_equal
    a, b = _data(31), _data(32)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    ts = _zero_copy(a)
    ts.index("mean", side.cuda_stream)
    probe, out_a = ts.alloc_runs(), ts.alloc_runs()
    torch.cuda.synchronize()                            # (the outputs' zero fill is on the default stream)
    ts.reduce("mean", probe, stream=side.cuda_stream)   # the track set's first launch is waited for whatever the caller asks
    for _ in range(3):
        ts.reduce("mean", out_a, stream=side.cuda_stream, sync=False)
    ts.close()
    ts_b = _zero_copy(b)
    ts_b.index("mean")
    out_b = ts_b.alloc_runs()
    ts_b.reduce("mean", out_b, sync=False)
    torch.cuda.synchronize()
    got_a, got_b = _got(out_a, 1), _got(out_b, 1)
    ts_b.close()
    assert_runs_equal(got_a, _expect(oracle, "d/a", a), 0.0, "the launch in flight at close()")
    assert_runs_equal(got_b, _expect(oracle, "d/b", b), 0.0, "the set that took its buffers")


def test_trim_empties_the_pools(oracle):
    """(e): nothing rests in either pool after wtamd_pool_trim, and the next set still works."""
    from helpers import assert_runs_equal
    from wiggletools_amd import _lib
    a = _data(11)
    _run(a)
    assert _stats()[2] > 0 and _stats()[5] > 0
    _lib.lib().wtamd_pool_trim()
    s = _stats()
    assert s[2] == 0 and s[5] == 0, s
    got, _ = _run(a)
    assert_runs_equal(got, _expect(oracle, "a", a), 0.0, "after the trim")
