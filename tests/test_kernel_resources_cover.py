"""Registers and scratch memory of the coverage / union kernels (csrc/wt_cover.hip), read off the cross-compiled gfx950 code
object as tests/test_kernel_resources.py does: fourteen small passes, one lane per interval or eight items per lane, whose
counters and running sums must all stay in registers."""
from test_kernel_resources import _kernels


def test_cover_kernels_use_no_scratch():
    mine = {name: k for name, k in _kernels().items() if "wt_cover_kernel" in name}
    assert len(mine) == 14, sorted(mine)
    for name, k in mine.items():
        assert k["spill"] == 0 and k["scratch"] == 0, (name, k)
        assert k["max_wg"] == 256, (name, k)
