"""wtamd_TeeWiggleIterator and wtamd_toFile of the emulated drop-in library (tests/emu/build.py: csrc/wt_iter_abi.cpp without the
HIP units, so the host sweep of csrc/wt_text.h) over bulk, overlapping and popping children: the file byte for byte the text
the compiled reference printed (through tests/text_model.py), lists the compression rule merges, holdFire, a seek, wide values
(tests/text_dropin.py, which tests/test_text_dropin_gpu.py runs over the product)."""
import text_dropin
from emu import build as emu_build


def test_the_dropin_writers_on_the_host_sweep(tmp_path):
    text_dropin.check_dropin(text_dropin.DropIn(emu_build.build_dropin()), tmp_path)
