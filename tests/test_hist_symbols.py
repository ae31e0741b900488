"""The histogram's C ABI: the two doors and the drop-in's entry points are exported by the library and declared by
include/wiggletools_amd.h, the flags are defined, and the Python mirror has its names (no compute call is made here)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wtamd_runs_histogram", "wtamd_runs_histogram_host", "wtamd_histogram", "wtamd_normalize_histogram", "wtamd_print_histogram",
         "wtamd_histogram_width", "wtamd_histogram_count", "wtamd_histogram_row", "wtamd_histogram_range", "wtamd_destroy_histogram")


def test_the_library_exports_the_histogram_doors_and_the_dropin():
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
    assert re.search(r"#define WTAMD_HIST_RANGE_GIVEN\s+1u", txt) and re.search(r"#define WTAMD_HIST_ACCUMULATE\s+2u", txt)
    assert re.search(r"typedef struct wtamd_histogram_st wtamd_Histogram;", txt)
    from wiggletools_amd import dropin, engine
    assert all(hasattr(engine, f) for f in ("histogram_runlists", "_hist_door"))
    assert hasattr(dropin, "histogram")
    assert (engine.HIST_RANGE_GIVEN, engine.HIST_ACCUMULATE) == (1, 2)
