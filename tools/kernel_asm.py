#!/usr/bin/env python
"""ISA of ONE instantiation of wt_delta_kernel in seconds instead of the minute its unit takes: the kernel's header, one explicit
instantiation, hipcc -S.   tools/kernel_asm.py 10 0 [-DFLAG ...] > /tmp/k.s
(10 = WT_OP_TTEST, 2 = mean, 6 = stddev ...; second argument: DF)"""
import os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
op, df = sys.argv[1], sys.argv[2]
flags = sys.argv[3:]
text = ('#include "%s"\ntemplate __global__ void wt_delta_kernel<%s, %s>(const WtParams);\n' %
        (os.path.join(ROOT, "wiggletools_amd/csrc/wt_delta_kernel.h"), op, "true" if df != "0" else "false"))
with tempfile.TemporaryDirectory() as d:
    name, out = os.path.join(d, "k.hip"), os.path.join(d, "k.s")
    open(name, "w").write(text)
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-function", "-Wno-pass-failed",
                           "--cuda-device-only", "-S", name, "-o", out] + flags)
    sys.stdout.write(open(out).read())
