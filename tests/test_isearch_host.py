"""The window index's lane search (csrc/wt_isearch.h) on the host: tests/isearch_fuzz.cpp, a stand-alone program built with
-fsanitize=address,undefined, includes the header as plain C++ and fuzzes the interpolation search against std::lower_bound
-- brackets of 0 to 40 000 entries; the bench's distribution, all entries equal, 99 % of the runs in the first 1 % of the
coordinates, boundaries on / next to / outside the entries, guesses at both ends, coordinates up to WTAMD_MAX_COORD -- with
every read of finish[] counted: at most 2 ceil(log2 n) + 6 of them on any input, and on the bench's shape (64 boundaries over
a bracket of 32 768 runs) strictly fewer on average than the routine it replaces (kept in the program as the baseline).
Measured: baseline 11.113 reads per search, interpolation 5.045."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_isearch_fuzz_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "isearch_fuzz")
    # the sanitizers' runtimes inside the program: it runs the same whatever else the environment loads into a process
    static = ["-static-libasan", "-static-libubsan"] if cxx.endswith("g++") else ["-static-libsan"]
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror"] + static + [
                           os.path.join(HERE, "isearch_fuzz.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "isearch-fuzz-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    m = re.search(r"mean reads: baseline ([0-9.]+) interpolation ([0-9.]+)", r.stdout)
    assert m and float(m.group(2)) < float(m.group(1)), r.stdout
