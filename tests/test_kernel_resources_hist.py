"""Registers and scratch memory of the histogram unit's kernels (csrc/wt_hist.hip), read off the cross-compiled gfx950 code
object as tests/test_kernel_resources_units.py does: five passes (range, load, bins in LDS, bins in global memory, finish) whose
keys, columns and wave sums must all stay in registers, with the row's counters (32 KiB) in LDS."""
from test_kernel_resources import _kernels


def test_hist_kernels_use_no_scratch():
    mine = {name: k for name, k in _kernels().items() if "wt_hist_kernel" in name}
    assert len(mine) == 5, sorted(mine)
    for name, k in mine.items():
        assert k["spill"] == 0 and k["scratch"] == 0, (name, k)
        assert k["max_wg"] == 256, (name, k)
