"""The energy door's C ABI: the two doors and the drop-in's entry points are exported by the library and declared by
include/wiggletools_amd.h, and the Python mirror has its names (no compute call is made here)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wtamd_runs_energy", "wtamd_runs_energy_host", "wtamd_energy_finish", "wtamd_EnergyIntegrator", "wtamd_EnergySpectrum")


def test_the_library_exports_the_energy_doors_and_the_dropin():
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
    assert all(hasattr(engine, f) for f in ("energy_runlists", "_energy_door"))
    assert all(hasattr(dropin, f) for f in ("energy_integrator", "energy_spectrum"))
