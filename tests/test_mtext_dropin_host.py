"""wtamd_TeeMultiplexer, wtamd_toStdoutMultiplexer and wtamd_PasteMultiplexer of the emulated drop-in library (tests/emu/build.py:
csrc/wt_iter_abi.cpp without the HIP units, so the host sweep wtm_host of csrc/wt_mtext.h) over this library's Multiplexer and
over wtamd_ApplyMultiplexer: the file byte for byte the model's text of the rows served, the rows unchanged, 25000 rows,
holdFire, a seek mid-block, paste, stdout and the short infile (tests/mtext_dropin.py, which tests/test_mtext_dropin_gpu.py runs
over the product)."""
import mtext_dropin
from emu import build as emu_build


def test_the_multiplexer_writers_on_the_host_sweep(tmp_path):
    mtext_dropin.check_dropin(mtext_dropin.DropIn(emu_build.build_dropin()), tmp_path)


def test_stdout_and_the_short_infile_in_child_processes(tmp_path):
    mtext_dropin.check_children(emu_build.build_dropin(), tmp_path)
