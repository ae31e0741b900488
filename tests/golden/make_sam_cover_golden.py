#!/usr/bin/env python
"""Generates tests/golden/sam_cover_fixtures.json: what the compiled reference's SamReader (src/samReader.c, pile-up mode) pops
over SAM text, next to the covering components of that text's reads in FILE order -- the input wtamd_runs_coverage_flags
takes with WTAMD_COVER_ANY_ORDER (tests/test_cover_any_order_emu.py, tests/test_cover_any_order_gpu.py).

The driver is our own: it opens SamReader on a file, pops it to the end and prints every record.  It is compiled together
with the reference's sources, unmodified and from where they lie, into a shared object in a temporary directory.  Nothing
compiled is kept.

The components follow samReader.c:45-76, :106-112: a CIGAR is a sequence of blocks `count op` walked with a cursor that
starts at the read's position; M, X, = and D give [cursor, cursor + count) and advance the cursor, N only advances it, I, S,
H and P do neither, `*` gives nothing.  A segment is a maximal stretch of lines with one name (field 3).  The generator
asserts for every case that the reference's pops equal the coverage model (tests/cover_model.py) over every segment's
components sorted by start, record for record.

Cases: the reference's own test/sam.sam (recorded as components, not as text), and a hand-made text with every op, `*`,
multi-component reads followed by earlier starts, touching reads, several names, identical positions.

Run where the reference's sources are present:  python tests/golden/make_sam_cover_golden.py <path to the reference>
"""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cover_model as M  # noqa: E402
from make_coverage_golden import REF_SRCS  # noqa: E402

DRIVER = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "wiggletools.h"
#include "wiggleIterator.h"

long long golden_sam(char *path, long long cap, char *out) {
    char *buf = NULL;
    size_t len = 0;
    FILE *fp = open_memstream(&buf, &len);
    WiggleIterator *wi = SamReader(path, 0);
    while (!wi->done) {
        fprintf(fp, "%s\t%d\t%d\t%.17g\n", wi->chrom, wi->start, wi->finish, wi->value);
        pop(wi);
    }
    fclose(fp);
    if ((long long) len <= cap) memcpy(out, buf, len);
    free(buf);
    return (long long) len;
}
'''


def line(name, pos, cigar, k=[0]):
    k[0] += 1
    return "r%d\t0\t%s\t%d\t30\t%s\t*\t0\t0\tACGT\tIIII\n" % (k[0], name, pos, cigar)


def hand_made():
    rows = [("chr1", 100, "50M1000N50M"), ("chr1", 120, "10M2I5D10M"), ("chr1", 120, "3S20M"), ("chr1", 130, "*"),
            ("chr1", 143, "4=1X"), ("chr1", 148, "5H10M3P7M2S"), ("chr1", 165, "5M"), ("chr1", 170, "5M"), ("chr1", 170, "5M"),
            ("chr1", 900, "20M300N20M40N20M"), ("chr1", 905, "30M"), ("chr1", 1160, "10M"), ("chr1", 5000, "7I"),
            ("chr2", 5, "10M"), ("chr2", 15, "10M"), ("chr2", 15, "2M3D2M3N4M"), ("chr2", 4000, "25M"),
            ("chr20", 1, "1M"), ("chr21", 10, "12M80N12M"), ("chr21", 11, "12M"), ("chr21", 95, "30M")]
    return "".join(line(*r) for r in rows)


def components(text):
    """(names, per segment (start, finish)) of SAM text, components in line order and in CIGAR order inside a line."""
    names, segs = [], []
    for ln in text.splitlines():
        if ln.startswith("#"):
            continue
        fld = ln.split("\t")
        name, pos, cigar = fld[2], int(fld[3]), fld[5]
        if not names or names[-1] != name:
            names.append(name)
            segs.append(([], []))
        if cigar == "*":
            continue
        assert re.fullmatch(r"([1-9][0-9]{0,8}[MIDNSHPX=])+", cigar), cigar
        cur = pos
        for count, op in re.findall(r"([0-9]+)([MIDNSHPX=])", cigar):
            if op in "MX=D":
                segs[-1][0].append(cur)
                segs[-1][1].append(cur + int(count))
            if op in "MX=DN":
                cur += int(count)
    return names, [(np.array(s, np.int32), np.array(f, np.int32)) for s, f in segs]


def build(ref, tmp):
    drv = os.path.join(tmp, "driver.c")
    open(drv, "w").write(DRIVER)
    so = os.path.join(tmp, "libsamgold.so")
    subprocess.check_call(["gcc", "-g", "-w", "-O3", "-std=gnu99", "-D_GNU_SOURCE", "-fPIC", "-shared", "-I" + os.path.join(ref, "src")] +
                          [os.path.join(ref, "src", s) for s in REF_SRCS] + [drv, "-o", so, "-lm", "-lpthread"])
    return C.CDLL(so, mode=os.RTLD_LAZY)


def pops(lib, path):
    cap = 1 << 24
    out = C.create_string_buffer(cap)
    lib.golden_sam.restype = C.c_longlong
    n = lib.golden_sam(path.encode(), C.c_longlong(cap), out)
    assert 0 <= n <= cap, n
    rows = [r.split("\t") for r in out.raw[:n].decode().splitlines()]
    return [(r[0], int(r[1]), int(r[2]), float(r[3])) for r in rows]


def main():
    ref = sys.argv[1]
    out = {"generator": "tests/golden/make_sam_cover_golden.py",
           "source": "compiled reference v1.2.11: SamReader(path, false) popped to the end; components by the rule of samReader.c:45-76", "cases": []}
    texts = {"sam.sam": open(os.path.join(ref, "test", "sam.sam")).read(), "hand_made": hand_made()}
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(ref, tmp)
        path = os.path.join(tmp, "in.sam")
        for name, text in texts.items():
            open(path, "w").write(text)
            got = pops(lib, path)
            names, segs = components(text)
            want = []
            for nm, (s, f) in zip(names, segs):
                o = np.argsort(s, kind="stable")
                cs, cf, cv = M.coverage(s[o], f[o])
                want += [(nm, int(a), int(b), float(v)) for a, b, v in zip(cs, cf, cv)]
            assert got == want, (name, len(got), len(want))
            out["cases"].append({"name": name, "seg_name": names, "seg_off": np.concatenate([[0], np.cumsum([len(s) for s, _ in segs])]).tolist(),
                                 "start": np.concatenate([s for s, _ in segs]).tolist(), "finish": np.concatenate([f for _, f in segs]).tolist(),
                                 "unsorted_segments": int(sum(bool(np.any(np.diff(s) < 0)) for s, _ in segs)),
                                 "pops": {"chrom": [r[0] for r in got], "start": [r[1] for r in got], "finish": [r[2] for r in got],
                                          "value": [r[3] for r in got]}})
            print(name, len(got), "pops,", sum(len(s) for s, _ in segs), "components,", out["cases"][-1]["unsorted_segments"], "unsorted segments")
    dst = os.path.join(HERE, "sam_cover_fixtures.json")
    with open(dst, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    size = os.path.getsize(dst)
    print("wrote %d cases, every pop equal to the model, %d bytes" % (len(out["cases"]), size))
    assert size < 250000, size


if __name__ == "__main__":
    main()
