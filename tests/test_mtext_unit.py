"""The C ABI of the tile-text unit (csrc/wt_mtext.hip, csrc/wt_abi_mtext.h): its doors and drop-in entry points are exported by
the library and declared by include/wiggletools_amd.h, its constants are defined, the Python mirror has its names, no
un-prefixed name of the reference's writer is exported (tests/test_mixed_link.py links the reference's own beside the library);
its kernels as the cross-compiled gfx950 code object holds them; and the drop-in emulator library depends on its header."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wtamd_tile_text", "wtamd_tile_text_host", "wtamd_trackset_mtext", "wtamd_trackset_mtext_host", "wtamd_TeeMultiplexer", "wtamd_toStdoutMultiplexer",
         "wtamd_PasteMultiplexer")
BARE = ("TeeMultiplexer", "PasteMultiplexer", "toStdoutMultiplexer")


@pytest.fixture(scope="module")
def library():
    import __graft_entry__ as g
    g.build()
    from wiggletools_amd import _lib
    return _lib.LIB_PATH


def test_the_library_exports_the_doors_and_the_dropin(library):
    lib = ctypes.CDLL(library)
    assert not [n for n in NAMES if not hasattr(lib, n)]


def test_no_unprefixed_name_of_the_reference_writer_is_exported(library):
    out = subprocess.check_output(["nm", "-D", "--defined-only", library]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [n for n in BARE if n in exported]
    assert all(n in exported for n in NAMES)


def test_the_header_declares_them_and_python_mirrors_them(library):
    txt = open(os.path.join(ROOT, "include", "wiggletools_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, txt), n
    for rx in (r"#define WTAMD_MTEXT_BEDGRAPH\s+1u", r"#define WTAMD_MTEXT_STRICT\s+2u", r"#define WTAMD_MTEXT_MAX_WIDTH\s+(\d+)\b"):
        assert re.search(rx, txt), rx
    assert int(re.search(r"#define WTAMD_MTEXT_MAX_WIDTH\s+(\d+)\b", txt).group(1)) >= 65536
    from wiggletools_amd import dropin, engine
    assert all(hasattr(engine, f) for f in ("tile_text", "_mtext_door", "MTEXT_BEDGRAPH", "MTEXT_STRICT")) and hasattr(engine.TrackSet, "mtext")
    assert all(hasattr(dropin, f) for f in ("tee_multiplexer", "to_stdout_multiplexer", "paste_multiplexer"))
    assert (engine.MTEXT_BEDGRAPH, engine.MTEXT_STRICT) == (1, 2)
    import mtext_model as M
    assert engine.MTEXT_MAX_WIDTH == M.MAX_WIDTH == int(re.search(r"#define WTM_MAX_WIDTH (\d+)\b", open(M.HEADER).read()).group(1))


def test_the_four_passes_keep_everything_in_registers():
    """The project's standing condition for side units: cells, mode, scan and emit are there, at 256 lanes, with no spilled
    register and no scratch memory -- the text is composed in the LDS window, never in a per-lane array."""
    from test_kernel_resources import _kernels
    mine = {name: k for name, k in _kernels().items() if "wt_mtext_kernel" in name}
    assert len(mine) == 4, sorted(mine)
    for name, k in mine.items():
        assert k["spill"] == 0 and k["scratch"] == 0 and k["max_wg"] == 256, (name, k)


def test_the_dropin_emulator_library_records_the_header():
    from emu import build as B
    deps = B.recorded_deps(B.build_dropin(), B.DROPIN_SOURCES)
    assert deps is not None and os.path.normpath(os.path.join(B.CSRC, "wt_mtext.h")) in set(deps)
