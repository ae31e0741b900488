"""Registers and scratch memory of the window unit's kernels (csrc/wt_window.hip), read off the cross-compiled gfx950 code
object as tests/test_kernel_resources_units.py does: seven passes (valid, count, cum, bins, heavy, ends, smooth) whose search
bounds, run cursors, window sums and NaN counts must all stay in registers, with the staged scanned counts (16 KiB), the
shares or the strips' values (34 KiB) in LDS."""
from test_kernel_resources import _kernels


def test_window_kernels_use_no_scratch():
    mine = {name: k for name, k in _kernels().items() if "wt_window_kernel" in name}
    assert len(mine) == 7, sorted(mine)
    for name, k in mine.items():
        assert k["spill"] == 0 and k["scratch"] == 0, (name, k)
        assert k["max_wg"] == 256, (name, k)
