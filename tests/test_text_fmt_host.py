"""The integer "%lf" of csrc/wt_text.h on the host: tests/text_fmt_fuzz.cpp, a stand-alone program built with
-fsanitize=address,undefined, includes the header as plain C++ and holds wtx_num / wtx_put_num against glibc's
snprintf("%f") -- every tie of the sixth decimal (N + j/128, odd j), both neighbours of 10^k - 5e-7, every power of two from
the smallest denormal to 2^64 with its neighbours, 2^53 +- 1 ulp, the largest narrow value, zeros, infinities and NaNs of
either sign, 1.5 million random mantissas under exponents 2^-80 .. 2^63 and a million random bit patterns below 2^64.  Every
byte and every length must be equal; there is no tolerance."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_text_fmt_fuzz_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "text_fmt_fuzz")
    # the sanitizers' runtimes inside the program: it runs the same whatever else the environment loads into a process
    static = ["-static-libasan", "-static-libubsan"] if cxx.endswith("g++") else ["-static-libsan"]
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
                           "-Wno-unused-function", "-Wno-unknown-pragmas"] + static + [os.path.join(HERE, "text_fmt_fuzz.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "text-fmt-fuzz-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    m = re.search(r"checked (\d+) values byte for byte, (\d+) wide", r.stdout)
    assert m and int(m.group(1)) >= 2500000 and int(m.group(2)) > 0, r.stdout
