"""Registers and scratch memory of the energy unit's kernels (csrc/wt_energy.hip), read off the cross-compiled gfx950 code
object as tests/test_kernel_resources_units.py does: three passes (last, main, final).  The main pass keeps a batch of runs, the
phases and the trigonometry in registers and its accumulators (32 KiB) in LDS."""
from test_kernel_resources import _kernels


def test_energy_kernels_use_no_scratch():
    mine = {name: k for name, k in _kernels().items() if "wt_energy_kernel" in name}
    assert len(mine) == 3, sorted(mine)
    for name, k in mine.items():
        assert k["spill"] == 0 and k["scratch"] == 0, (name, k)
        assert k["max_wg"] == 256, (name, k)
