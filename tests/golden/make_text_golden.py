#!/usr/bin/env python
"""Generates tests/golden/text_fixtures.json: what the compiled reference's TeeWiggleIterator (src/wigWriter.c:261-276; `write`
and `write_bg`) prints for every case of tests/text_model.py's reference_cases(), in both modes.

The driver is our own: the array-backed child iterator of make_apply_golden.py and a function that runs a TeeWiggleIterator
over it into an open_memstream and copies the text out.  It is compiled together with the reference's sources, unmodified and
from where they lie, into a shared object in a temporary directory.  Nothing compiled is kept.

The generator asserts for EVERY case, none left out, that the reference's text equals the model's byte for byte, and that the
compression rule the reference's wig writer puts in front leaves the list alone (so the door, which does not compress, is given
what the reference's printBlock was given).  The lists themselves are not stored: cases() builds them, and a digest of the input
is recorded beside the output.  Cases of up to 200 entries record the whole text; larger ones its SHA-256, its length and the
20 lines on either side of every block seam.

Run where the reference's sources are present:  python tests/golden/make_text_golden.py <path to the reference>
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import text_model as M  # noqa: E402
import make_apply_golden as AG  # noqa: E402
from make_coverage_golden import REF_SRCS  # noqa: E402

DRIVER = AG.DRIVER + r'''
#include <stdio.h>

/* Returns the text's length (above cap: too small). */
long long golden_text(int n_chrom, char **names, long long *seg_off, int *start, int *finish, double *value, int bedGraph,
                      long long cap, char *out) {
    char *buf = NULL;
    size_t len = 0;
    FILE *fp = open_memstream(&buf, &len);
    WiggleIterator *wi = arr_new(n_chrom, names, seg_off, start, finish, value, 0);
    runWiggleIterator(TeeWiggleIterator(wi, fp, bedGraph, false));
    fclose(fp);
    if ((long long) len <= cap) memcpy(out, buf, len);
    free(buf);
    return (long long) len;
}
'''


def build(ref, tmp):
    drv = os.path.join(tmp, "driver.c")
    open(drv, "w").write(DRIVER)
    so = os.path.join(tmp, "libtextgold.so")
    subprocess.check_call(["gcc", "-g", "-w", "-O3", "-std=gnu99", "-D_GNU_SOURCE", "-fPIC", "-shared", "-I" + os.path.join(ref, "src")] +
                          [os.path.join(ref, "src", s) for s in REF_SRCS] + [drv, "-o", so, "-lm", "-lpthread"])
    return C.CDLL(so, mode=os.RTLD_LAZY)


def run(lib, L, bedgraph):
    cap = 1 << 23
    out = C.create_string_buffer(cap)
    names = (C.c_char_p * len(L.names))(*L.names)
    seg = L.seg.astype("int64")
    p = lambda x: C.c_void_p(x.ctypes.data)      # noqa: E731
    lib.golden_text.restype = C.c_longlong
    n = lib.golden_text(C.c_int(len(L.names)), names, p(seg), p(L.s), p(L.f), p(L.v), C.c_int(bedgraph), C.c_longlong(cap), out)
    assert 0 < n <= cap, n
    return out.raw[:n]


def main():
    ref = sys.argv[1]
    out = {"generator": "tests/golden/make_text_golden.py",
           "source": "compiled reference v1.2.11: TeeWiggleIterator over array-backed children into a memory stream, wig and bedGraph mode",
           "cases": []}
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(ref, tmp)
        for name, L in M.reference_cases().items():
            assert M.same_lists(M.compress(L), L), (name, "the compression rule changes this list")
            assert len(set(L.names)) == len(L.names), name          # (the reference compares names, the door segments)
            for flags in (0, M.BEDGRAPH):
                txt = run(lib, L, flags)
                model = M.text(L, flags)[0]
                assert txt == model, (name, flags, len(txt), len(model))
                c = {"name": "%s/%d" % (name, flags), "case": name, "flags": flags, "entries": len(L), "input_sha256": L.digest(),
                     "bytes": len(txt), "sha256": hashlib.sha256(txt).hexdigest()}
                if len(L) <= 200:
                    c["text"] = txt.decode("latin-1")
                else:
                    c["seams"] = M.seam_lines(txt, L, flags)
                out["cases"].append(c)
    path = os.path.join(HERE, "text_fixtures.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    size = os.path.getsize(path)
    print("wrote %d texts, every one equal to the model byte for byte, %d bytes" % (len(out["cases"]), size))
    assert size < 250000, size
    for c in M.fixtures():                                  # what is stored reads back as what was recorded
        L = M.reference_cases()[c["case"]]
        M.check_against_fixture(c, L, c["flags"], M.text(L, c["flags"])[0])


if __name__ == "__main__":
    main()
