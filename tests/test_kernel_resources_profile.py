"""Registers and scratch memory of the profile kernels (csrc/wt_profile.hip), read off the cross-compiled gfx950 code object as
tests/test_kernel_resources.py does: seven passes (two validations, bounds, bins, heavy, fold, add) whose rounding searches,
bin sums and the eight rows of a fold must all stay in registers, with the dataset window (16 KiB) or the shares in LDS."""
from test_kernel_resources import _kernels


def test_profile_kernels_use_no_scratch():
    mine = {name: k for name, k in _kernels().items() if "wt_profile_kernel" in name}
    assert len(mine) == 7, sorted(mine)
    for name, k in mine.items():
        assert k["spill"] == 0 and k["scratch"] == 0, (name, k)
        assert k["max_wg"] == 256, (name, k)
