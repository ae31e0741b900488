"""wtamd_WiggleReader and wtamd_BedReader of the product, their chunks through wtamd_text_runs_host: pop for pop and through
wtamd_iterator_next_block what the compiled reference's readers popped, at the default chunk size and at chunks of 300 and of 8
bytes (WTAMD_READ_CHUNK_BYTES: cut inside sections and chromosomes; an irregular line in a later chunk falls over to the
reference-way reader and the file still reads as the reference reads it), seeks included, and MeanReduction over three text
files through the drop-in Multiplexer (tests/read_dropin.py, which tests/test_read_dropin_host.py runs over the emulated
library)."""
import os

import pytest

import read_dropin

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _pools_as_a_fresh_process_has_them():
    yield
    from wiggletools_amd import _lib
    _lib.lib().wtamd_pool_trim()


def _setenv(k, v):
    if v:
        os.environ[k] = v
    else:
        os.environ.pop(k, None)


def test_dropin(tmp_path):
    from wiggletools_amd import _lib
    _lib.lib()                                  # (PyTorch's HIP runtime goes first, whichever test file runs first: _lib.py)
    try:
        read_dropin.check_dropin(read_dropin.DropIn(_lib.LIB_PATH), tmp_path, _setenv)
    finally:
        _setenv("WTAMD_READ_CHUNK_BYTES", "")


def test_mean_over_three_text_files(tmp_path):
    from wiggletools_amd import _lib
    _lib.lib()
    read_dropin.check_mean(read_dropin.DropIn(_lib.LIB_PATH), tmp_path)


def test_the_python_mirrors(tmp_path):
    from wiggletools_amd import dropin
    import read_model as M
    wig, bed = tmp_path / "a.bg", tmp_path / "a.bed"
    wig.write_bytes(M.cases()["chrom_changes"][0])
    bed.write_bytes(M.cases()["bed_basic"][0])
    assert dropin.wiggle_reader(wig) and dropin.bed_reader(bed)
