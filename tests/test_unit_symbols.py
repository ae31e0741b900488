"""The C ABI of the window, histogram, energy and text units: each unit's doors and drop-in entry points are exported by the
library and declared by include/wiggletools_amd.h, its flags and constants are defined, and the Python mirror has its names
(no compute call is made here)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

UNITS = {
    # unit: names = the exported functions; header = regexes the header (without its comments) matches; engine / dropin = attributes
    # of the Python mirror; constants = {attribute of engine: value}
    "window": dict(
        names=("wtamd_runs_bin", "wtamd_runs_smooth", "wtamd_runs_bin_host", "wtamd_runs_smooth_host", "wtamd_BinIterator", "wtamd_SmoothIterator"),
        header=(),
        engine=("bin_runlists", "smooth_runlists", "_window_door"),
        dropin=("bin_iterator", "smooth_iterator"),
        constants={}),
    "hist": dict(
        names=("wtamd_runs_histogram", "wtamd_runs_histogram_host", "wtamd_histogram", "wtamd_normalize_histogram", "wtamd_print_histogram",
               "wtamd_histogram_width", "wtamd_histogram_count", "wtamd_histogram_row", "wtamd_histogram_range", "wtamd_destroy_histogram"),
        header=(r"#define WTAMD_HIST_RANGE_GIVEN\s+1u", r"#define WTAMD_HIST_ACCUMULATE\s+2u", r"typedef struct wtamd_histogram_st wtamd_Histogram;"),
        engine=("histogram_runlists", "_hist_door"),
        dropin=("histogram",),
        constants={"HIST_RANGE_GIVEN": 1, "HIST_ACCUMULATE": 2}),
    "energy": dict(
        names=("wtamd_runs_energy", "wtamd_runs_energy_host", "wtamd_energy_finish", "wtamd_EnergyIntegrator", "wtamd_EnergySpectrum"),
        header=(),
        engine=("energy_runlists", "_energy_door"),
        dropin=("energy_integrator", "energy_spectrum"),
        constants={}),
    "text": dict(
        names=("wtamd_runs_text", "wtamd_runs_text_host", "wtamd_TeeWiggleIterator", "wtamd_toFile", "wtamd_toStdout"),
        header=(r"#define WTAMD_TEXT_BEDGRAPH\s+1u", r"#define WTAMD_TEXT_BLOCK\s+10000\b"),
        engine=("text_runlists", "_text_door", "TextState"),
        dropin=("tee_iterator", "to_file", "to_stdout"),
        constants={"TEXT_BEDGRAPH": 1, "TEXT_BLOCK": 10000}),
}


@pytest.fixture(scope="module")
def library():
    import __graft_entry__ as g
    g.build()
    from wiggletools_amd import _lib
    return ctypes.CDLL(_lib.LIB_PATH)


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_the_library_exports_the_doors_and_the_dropin(library, unit):
    missing = [n for n in UNITS[unit]["names"] if not hasattr(library, n)]
    assert not missing, missing


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_the_header_declares_them(library, unit):
    u = UNITS[unit]
    txt = open(os.path.join(ROOT, "include", "wiggletools_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for n in u["names"]:
        assert re.search(r"\b%s\s*\(" % n, txt), n
    for rx in u["header"]:
        assert re.search(rx, txt), rx
    from wiggletools_amd import dropin, engine
    assert all(hasattr(engine, f) for f in u["engine"])
    assert all(hasattr(dropin, f) for f in u["dropin"])
    for name, value in u["constants"].items():
        assert getattr(engine, name) == value, name
    if unit == "text":
        assert ctypes.sizeof(engine.TextState) == 16


def test_the_text_state_is_16_bytes_to_a_c_compiler(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include "wiggletools_amd.h"\n_Static_assert(sizeof(wtamd_text_state) == 16, "wtamd_text_state");\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
