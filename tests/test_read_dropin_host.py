"""wtamd_WiggleReader and wtamd_BedReader of the emulated drop-in library (tests/emu/build.py: csrc/wt_iter_abi.cpp without the
HIP units, so the reference-way reader of csrc/wt_read.h) and again with WTAMD_NO_DEVICE_READ=1: pop for pop and block for
block what the compiled reference's readers popped, seeks included, irregular lines as the reference reads them or gives up on
them (exit status and message), and in front of MeanReduction (tests/read_dropin.py, which tests/test_read_dropin_gpu.py runs
over the product)."""
import os

import read_dropin
from emu import build as emu_build


def _setenv(k, v):
    if v:
        os.environ[k] = v
    else:
        os.environ.pop(k, None)


def test_the_dropin_readers_on_the_host(tmp_path):
    D = read_dropin.DropIn(emu_build.build_dropin())
    try:
        for no_device in ("", "1"):
            _setenv("WTAMD_NO_DEVICE_READ", no_device)
            read_dropin.check_dropin(D, tmp_path, _setenv, chunks=("", "300") if no_device else ("", "300", "8"))
    finally:
        _setenv("WTAMD_NO_DEVICE_READ", "")
        _setenv("WTAMD_READ_CHUNK_BYTES", "")


def test_in_front_of_mean_reduction(tmp_path):
    read_dropin.check_mean(read_dropin.DropIn(emu_build.build_dropin()), tmp_path)


def test_the_texts_the_reference_gives_up_on(tmp_path):
    read_dropin.run_exits(emu_build.build_dropin(), tmp_path)
