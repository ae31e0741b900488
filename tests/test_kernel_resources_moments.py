"""Registers and scratch memory of the run-moments kernels (csrc/wt_moments.hip), read off the cross-compiled gfx950 code
object as tests/test_kernel_resources.py does: the pass streams 16 bytes per run and must keep its accumulators -- three
sums, a pivot, two extremes with their run indices -- in registers."""
from test_kernel_resources import _kernels


def test_moments_kernels_use_no_scratch():
    mine = {name: k for name, k in _kernels().items() if "wt_moments_kernel" in name or "wt_moments_final_kernel" in name}
    assert len(mine) == 2, sorted(mine)
    for name, k in mine.items():
        assert k["spill"] == 0 and k["scratch"] == 0, (name, k)
