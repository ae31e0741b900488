"""Registers and scratch memory of the text unit's kernels (csrc/wt_text.hip), read off the cross-compiled gfx950 code object as
tests/test_kernel_resources_units.py does: three passes (measure, scan, emit) whose digits, byte counts and modes must all stay
in registers -- the text is composed in the LDS window, never in a per-lane array."""
from test_kernel_resources import _kernels


def test_text_kernels_use_no_scratch():
    mine = {name: k for name, k in _kernels().items() if "wt_text_kernel" in name}
    assert len(mine) == 3, sorted(mine)
    for name, k in mine.items():
        assert k["spill"] == 0 and k["scratch"] == 0, (name, k)
        assert k["max_wg"] == 256, (name, k)
