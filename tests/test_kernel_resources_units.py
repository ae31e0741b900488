"""Registers and scratch memory of the side units' kernels, read off the cross-compiled gfx950 code object as
tests/test_kernel_resources.py does (extracted once for this module): every instantiation a unit is meant to have is there,
and none keeps anything in scratch memory."""
import pytest

from test_kernel_resources import _kernels

UNITS = {
    # unit: (kernel names, instantiations, max_flat_workgroup_size or None where it is not pinned)
    # csrc/wt_apply.hip: five passes (two validations, bounds, chunk, final) whose search bounds, pivoted sums and merges must all
    # stay in registers, with the dataset window (16 KiB) or the lanes' partials (16 KiB) in LDS
    "apply": (("wt_apply_kernel",), 5, 256),
    # csrc/wt_cover.hip: fourteen small passes, one lane per interval or eight items per lane, whose counters and running sums
    # must all stay in registers
    "cover": (("wt_cover_kernel",), 14, 256),
    # csrc/wt_energy.hip: three passes (last, main, final).  The main pass keeps a batch of runs, the phases and the trigonometry
    # in registers and its accumulators (32 KiB) in LDS
    "energy": (("wt_energy_kernel",), 3, 256),
    # csrc/wt_hist.hip: five passes (range, load, bins in LDS, bins in global memory, finish) whose keys, columns and wave sums
    # must all stay in registers, with the row's counters (32 KiB) in LDS
    "hist": (("wt_hist_kernel",), 5, 256),
    # csrc/wt_profile.hip: seven passes (two validations, bounds, bins, heavy, fold, add) whose rounding searches, bin sums and
    # the eight rows of a fold must all stay in registers, with the dataset window (16 KiB) or the shares in LDS
    "profile": (("wt_profile_kernel",), 7, 256),
    # csrc/wt_region.hip: three passes whose search bounds, counts and output offsets must all stay in registers, with the mask
    # window (16 KiB) and the lanes' counts in LDS
    "region": (("wt_region_kernel",), 3, 256),
    # csrc/wt_moments.hip: the pass streams 16 bytes per run and must keep its accumulators -- three sums, a pivot, two extremes
    # with their run indices -- in registers
    "moments": (("wt_moments_kernel", "wt_moments_final_kernel"), 2, None),
    # csrc/wt_text.hip: three passes (measure, scan, emit) whose digits, byte counts and modes must all stay in registers -- the
    # text is composed in the LDS window, never in a per-lane array
    "text": (("wt_text_kernel",), 3, 256),
    # csrc/wt_window.hip: seven passes (valid, count, cum, bins, heavy, ends, smooth) whose search bounds, run cursors, window sums
    # and NaN counts must all stay in registers, with the staged scanned counts (16 KiB), the shares or the strips' values
    # (34 KiB) in LDS
    "window": (("wt_window_kernel",), 7, 256),
}


@pytest.fixture(scope="module")
def kernels():
    return _kernels()


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_unit_kernels_use_no_scratch(kernels, unit):
    names, count, max_wg = UNITS[unit]
    mine = {name: k for name, k in kernels.items() if any(n in name for n in names)}
    assert len(mine) == count, sorted(mine)
    for name, k in mine.items():
        assert k["spill"] == 0 and k["scratch"] == 0, (name, k)
        if max_wg is not None:
            assert k["max_wg"] == max_wg, (name, k)
