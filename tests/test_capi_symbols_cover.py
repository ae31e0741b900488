"""The coverage entries with flags are declared in include/wiggletools_amd.h and exported by the library, on a GPU-less host
(no compute call is made here); the flag's value is the one the kernels' header and the Python mirror use."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flags_entries_are_declared_and_exported():
    import __graft_entry__ as g
    g.build()
    from wiggletools_amd import _lib, engine
    txt = open(os.path.join(ROOT, "include", "wiggletools_amd.h")).read()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("wtamd_runs_coverage_flags", "wtamd_runs_coverage_host_flags", "wtamd_runs_coverage", "wtamd_runs_coverage_host"):
        assert re.search(r"\bint %s\s*\(" % name, txt), name
        assert hasattr(L, name), name
    flag = int(re.search(r"#define WTAMD_COVER_ANY_ORDER (\d+)u", txt).group(1))
    hdr = open(os.path.join(ROOT, "wiggletools_amd", "csrc", "wt_cover.h")).read()
    assert flag == int(re.search(r"#define WCV_ANY_ORDER (\d+)u", hdr).group(1)) == engine.COVER_ANY_ORDER
