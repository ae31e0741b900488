"""Registers and scratch memory of the apply kernels (csrc/wt_apply.hip), read off the cross-compiled gfx950 code object as
tests/test_kernel_resources.py does: five passes (two validations, bounds, chunk, final) whose search bounds, pivoted sums and
merges must all stay in registers, with the dataset window (16 KiB) or the lanes' partials (16 KiB) in LDS."""
from test_kernel_resources import _kernels


def test_apply_kernels_use_no_scratch():
    mine = {name: k for name, k in _kernels().items() if "wt_apply_kernel" in name}
    assert len(mine) == 5, sorted(mine)
    for name, k in mine.items():
        assert k["spill"] == 0 and k["scratch"] == 0, (name, k)
        assert k["max_wg"] == 256, (name, k)
