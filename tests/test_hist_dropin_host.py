"""wtamd_histogram, wtamd_normalize_histogram and wtamd_print_histogram of the emulated drop-in library (tests/emu/build.py:
csrc/wt_iter_abi.cpp without the HIP units, so the host sweep of csrc/wt_hist.h) over bulk and popping children: the recorded
matrices, ranges and texts (tests/hist_dropin.py, which tests/test_hist_gpu.py runs over the product)."""
import hist_dropin
import hist_model as M
from emu import build as emu_build


def test_the_dropin_histogram_on_the_host_sweep():
    hist_dropin.check_dropin(hist_dropin.DropIn(emu_build.build_dropin()), M.fixtures())
