"""wtamd_TeeMultiplexer, wtamd_toStdoutMultiplexer and wtamd_PasteMultiplexer of the product over this library's Multiplexer and
over wtamd_ApplyMultiplexer, with the device door and again with WTAMD_NO_DEVICE_MTEXT=1: the same bytes (tests/mtext_dropin.py,
which tests/test_mtext_dropin_host.py runs over the emulated drop-in library); the Python wrappers."""
import os

import pytest

import mtext_dropin
import mtext_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _pools_as_a_fresh_process_has_them():
    """The staging buffers of these tests rest in the library's process-wide pools afterwards; tests that count the pools'
    misses (tests/test_trackset_pool.py) expect to meet nothing larger than their own buffers there."""
    yield
    from wiggletools_amd import _lib
    _lib.lib().wtamd_pool_trim()


def test_dropin(tmp_path):
    from wiggletools_amd import _lib
    _lib.lib()                                  # (PyTorch's HIP runtime goes first, whichever test file runs first: _lib.py)

    def setenv(k, v):
        os.environ[k] = v

    try:
        mtext_dropin.check_dropin(mtext_dropin.DropIn(_lib.LIB_PATH), tmp_path, setenv)
    finally:
        os.environ.pop("WTAMD_NO_DEVICE_MTEXT", None)


def test_stdout_and_the_short_infile_in_child_processes(tmp_path):
    from wiggletools_amd import _lib
    _lib.lib()
    mtext_dropin.check_children(_lib.LIB_PATH, tmp_path, amd=True)


def test_python_dropin_tee_and_paste(tmp_path):
    from wiggletools_amd import _lib, dropin
    _lib.lib()
    D = mtext_dropin.DropIn(_lib.LIB_PATH)
    rl = mtext_dropin.small_tracks()
    rows = D.read_mux(D.tracks(rl))
    m, close = dropin.tee_multiplexer(D.tracks(rl), tmp_path / "t.wig")
    assert mtext_dropin.same_rows(D.read_mux(m), rows)
    close()
    assert open(tmp_path / "t.wig", "rb").read() == M.text(mtext_dropin.tile_of(rows), 0)[0]
    with open(tmp_path / "in.txt", "w") as fh:
        fh.write("".join("line %d\n" % i for i in range(len(rows))))
    m, close = dropin.paste_multiplexer(D.tracks(rl), tmp_path / "in.txt", tmp_path / "p.txt")
    D.read_mux(m)
    close()
    assert open(tmp_path / "p.txt", "rb").read() == M.text(mtext_dropin.tile_of(rows, [b"line %d" % i for i in range(len(rows))]), 0)[0]
