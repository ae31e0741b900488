"""The number parser of csrc/wt_read.h on the host: tests/read_num_fuzz.cpp, a stand-alone program built with
-fsanitize=address,undefined, includes the header as plain C++ and holds wtr_number against glibc's strtod bit for bit -- every
digit count 1 .. 20 with the point at every place, exponents -30 .. 30 in every spelling, W = 2^53 and its neighbours, fractions
with trailing zeros, "%f", "%.6g" and "%.17g" of a million random doubles -- and every numeral the parser calls slow to lie
truly outside the exact set.  There is no tolerance."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_read_num_fuzz_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "read_num_fuzz")
    # the sanitizers' runtimes inside the program: it runs the same whatever else the environment loads into a process
    static = ["-static-libasan", "-static-libubsan"] if cxx.endswith("g++") else ["-static-libsan"]
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                           "-Werror", "-Wno-unused-function", "-Wno-unknown-pragmas"] + static + [os.path.join(HERE, "read_num_fuzz.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "read-num-fuzz-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    m = re.search(r"checked (\d+) exact numerals bit for bit, (\d+) slow", r.stdout)
    assert m and int(m.group(1)) >= 2000000 and int(m.group(2)) >= 500000, r.stdout
