"""Registers and scratch memory of the region kernels (csrc/wt_region.hip), read off the cross-compiled gfx950 code object as
tests/test_kernel_resources.py does: three passes whose search bounds, counts and output offsets must all stay in registers,
with the mask window (16 KiB) and the lanes' counts in LDS."""
from test_kernel_resources import _kernels


def test_region_kernels_use_no_scratch():
    mine = {name: k for name, k in _kernels().items() if "wt_region_kernel" in name}
    assert len(mine) == 3, sorted(mine)
    for name, k in mine.items():
        assert k["spill"] == 0 and k["scratch"] == 0, (name, k)
        assert k["max_wg"] == 256, (name, k)
