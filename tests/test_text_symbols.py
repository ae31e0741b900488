"""The text unit's C ABI: the two doors and the drop-in's entry points are exported by the library and declared by
include/wiggletools_amd.h, the flag and the block length are defined, wtamd_text_state is 16 bytes, and the Python mirror has
its names (no compute call is made here)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wtamd_runs_text", "wtamd_runs_text_host", "wtamd_TeeWiggleIterator", "wtamd_toFile", "wtamd_toStdout")


def test_the_library_exports_the_text_doors_and_the_dropin():
    import __graft_entry__ as g
    g.build()
    from wiggletools_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in NAMES if not hasattr(L, n)]
    assert not missing, missing


def test_the_header_declares_them(tmp_path):
    txt = open(os.path.join(ROOT, "include", "wiggletools_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, txt), n
    assert re.search(r"#define WTAMD_TEXT_BEDGRAPH\s+1u", txt) and re.search(r"#define WTAMD_TEXT_BLOCK\s+10000\b", txt)
    from wiggletools_amd import dropin, engine
    assert all(hasattr(engine, f) for f in ("text_runlists", "_text_door", "TextState"))
    assert all(hasattr(dropin, f) for f in ("tee_iterator", "to_file", "to_stdout"))
    assert (engine.TEXT_BEDGRAPH, engine.TEXT_BLOCK) == (1, 10000)
    assert ctypes.sizeof(engine.TextState) == 16


def test_the_state_is_16_bytes_to_a_c_compiler(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include "wiggletools_amd.h"\n_Static_assert(sizeof(wtamd_text_state) == 16, "wtamd_text_state");\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
