"""The window operators' C ABI: the four doors and the two constructors are exported by the library and declared by
include/wiggletools_amd.h (no compute call is made here)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wtamd_runs_bin", "wtamd_runs_smooth", "wtamd_runs_bin_host", "wtamd_runs_smooth_host", "wtamd_BinIterator", "wtamd_SmoothIterator")


def test_the_library_exports_the_window_doors_and_constructors():
    import __graft_entry__ as g
    g.build()
    from wiggletools_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in NAMES if not hasattr(L, n)]
    assert not missing, missing


def test_the_header_declares_them():
    txt = open(os.path.join(ROOT, "include", "wiggletools_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, txt), n
    from wiggletools_amd import dropin, engine
    assert all(hasattr(engine, f) for f in ("bin_runlists", "smooth_runlists", "_window_door"))
    assert all(hasattr(dropin, f) for f in ("bin_iterator", "smooth_iterator"))
