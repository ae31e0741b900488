#!/usr/bin/env python
"""Generates tests/golden/read_fixtures.json: what the compiled reference's WiggleReader (src/wigReader.c) and BedReader
(src/bedReader.c) pop for every regular case of tests/read_model.py's cases(), and how BedReader ends on the unsorted cases.

The driver is our own: it opens a reader on a temporary file, pops it to the end and prints every record as name, start,
finish, the bits of the value and the name with its length (a name may hold a newline).  It is compiled together with the reference's sources, unmodified and from where they lie,
into a shared object in a temporary directory.  Nothing compiled is kept.

The generator asserts for EVERY case, none left out, that the reference's records equal the model's (read_model.
reference_reading: the model's records, slow values through float(), behind the compression rule for a wig reader).  Cases of up
to 300 records are recorded whole; larger ones as a digest, the count and the eight records at either end.  The unsorted BED
cases run in a forked child: exit status and stderr are recorded as data.

Run where the reference's sources are present:  python tests/golden/make_read_golden.py <path to the reference>
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
import read_model as M  # noqa: E402
from make_coverage_golden import REF_SRCS  # noqa: E402

DRIVER = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "wiggletools.h"
#include "wiggleIterator.h"

static void golden_pops(WiggleIterator *wi, FILE *fp);

/* into the file at outpath (what was popped survives an exit(1) of the reader: exit flushes it); pops >= 0: that many pop()
 * calls, then a seek to (chrom, start, finish), then to the end */
void golden_read_file(char *path, int bed, char *outpath, int pops, char *chrom, int start, int finish) {
    FILE *fp = fopen(outpath, "w");
    WiggleIterator *wi = bed ? BedReader(path) : WiggleReader(path);
    if (pops >= 0) {
        for (int k = 0; k < pops && !wi->done; k++) pop(wi);
        seek(wi, chrom, start, finish);
    }
    golden_pops(wi, fp);
    fclose(fp);
}

static void golden_pops(WiggleIterator *wi, FILE *fp) {
    while (!wi->done) {
        unsigned long long bits;
        memcpy(&bits, &wi->value, 8);
        fprintf(fp, "%d\t%d\t%016llx\t%d\t%s\n", wi->start, wi->finish, bits, (int) strlen(wi->chrom), wi->chrom);
        pop(wi);
    }
}

long long golden_read(char *path, int bed, long long cap, char *out) {
    char *buf = NULL;
    size_t len = 0;
    FILE *fp = open_memstream(&buf, &len);
    WiggleIterator *wi = bed ? BedReader(path) : WiggleReader(path);
    while (!wi->done) {
        unsigned long long bits;
        memcpy(&bits, &wi->value, 8);
        fprintf(fp, "%d\t%d\t%016llx\t%d\t%s\n", wi->start, wi->finish, bits, (int) strlen(wi->chrom), wi->chrom);
        pop(wi);
    }
    fclose(fp);
    if ((long long) len <= cap) memcpy(out, buf, len);
    free(buf);
    return (long long) len;
}
'''


def build(ref, tmp):
    drv = os.path.join(tmp, "driver.c")
    open(drv, "w").write(DRIVER)
    so = os.path.join(tmp, "libreadgold.so")
    subprocess.check_call(["gcc", "-g", "-w", "-O3", "-std=gnu99", "-D_GNU_SOURCE", "-fPIC", "-shared", "-I" + os.path.join(ref, "src")] +
                          [os.path.join(ref, "src", s) for s in REF_SRCS] + [drv, "-o", so, "-lm", "-lpthread"])
    return C.CDLL(so, mode=os.RTLD_LAZY)


def run(lib, path, bed):
    cap = 1 << 24
    out = C.create_string_buffer(cap)
    lib.golden_read.restype = C.c_longlong
    n = lib.golden_read(path.encode(), C.c_int(bed), C.c_longlong(cap), out)
    assert 0 <= n <= cap, n
    return parse(out.raw[:n])


def parse(raw):
    recs, p, n = [], 0, len(raw)
    while p < n:                                # start, finish, bits, the name's length, the name (it may hold a newline)
        q = p
        for _ in range(4):
            q = raw.index(b"\t", q) + 1
        a, b, bits, ln = raw[p:q - 1].split(b"\t")
        recs.append((raw[q:q + int(ln)], int(a), int(b), int(bits, 16)))
        p = q + int(ln) + 1
    return recs


def run_file(lib, path, bed, outpath, seek=None):
    pops, chrom, a, b = seek if seek else (-1, b"", 0, 0)
    lib.golden_read_file.restype = None
    lib.golden_read_file(path.encode(), C.c_int(bed), outpath.encode(), C.c_int(pops), chrom, C.c_int(a), C.c_int(b))
    return parse(open(outpath, "rb").read())


def in_child(tmp, path, call):
    """call() in a forked child with stderr in a file: (exit status, stderr)."""
    errpath = os.path.join(tmp, "err.txt")
    sys.stdout.flush()
    pid = os.fork()
    if pid == 0:
        os.dup2(os.open(errpath, os.O_WRONLY | os.O_CREAT | os.O_TRUNC), 2)
        call()
        os._exit(0)
    status = os.waitpid(pid, 0)[1]
    assert os.WIFEXITED(status), status
    return os.WEXITSTATUS(status), open(errpath, "rb").read().decode("latin-1").replace(path, "<path>")


def main():
    ref = sys.argv[1]
    out = {"generator": "tests/golden/make_read_golden.py",
           "source": "compiled reference v1.2.11: WiggleReader / BedReader over a temporary file, popped to the end", "cases": [], "unsorted": []}
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(ref, tmp)
        path = os.path.join(tmp, "in.txt")
        for name, (data, flags) in M.cases().items():
            open(path, "wb").write(data)
            got = run(lib, path, 1 if flags & M.BED else 0)
            want = M.reference_reading(data, flags)
            if got != want:
                k = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
                raise AssertionError((name, len(got), len(want), k, got[k:k + 2], want[k:k + 2]))
            c = {"name": name, "flags": flags, "input_sha256": hashlib.sha256(data).hexdigest(), "bytes": len(data)}
            c.update(M.as_fixture(got))
            out["cases"].append(c)
        for name, (data, n_unsorted) in M.unsorted_cases().items():
            open(path, "wb").write(data)
            errpath = os.path.join(tmp, "err.txt")
            sys.stdout.flush()
            pid = os.fork()
            if pid == 0:
                os.dup2(os.open(errpath, os.O_WRONLY | os.O_CREAT | os.O_TRUNC), 2)
                run(lib, path, 1)
                os._exit(0)
            status = os.waitpid(pid, 0)[1]
            assert os.WIFEXITED(status) and os.WEXITSTATUS(status) == 1, (name, status)
            assert M.read(data, M.BED).counts["n_unsorted"] >= 1
            out["unsorted"].append({"name": name, "input_sha256": hashlib.sha256(data).hexdigest(), "exit_status": 1,
                                    "stderr": open(errpath).read().replace(path, "<path>")})
        # seeks: after `pops` pop() calls, to a window; the sequence from there to the end
        out["seeks"] = []
        for name, (pops, chrom, a, b) in M.seek_cases().items():
            data, flags = M.cases()[name.split("/")[0]]
            open(path, "wb").write(data)
            outpath = os.path.join(tmp, "out.txt")
            status, err = in_child(tmp, path, lambda: run_file(lib, path, 1 if flags & M.BED else 0, outpath, (pops, chrom, a, b)))
            assert status == 0, (name, status, err)    # (a BED window that clips a start makes the reference call the file unsorted: not here)
            got = parse(open(outpath, "rb").read())
            c = {"name": name, "case": name.split("/")[0], "pops": pops, "chrom": chrom.decode(), "start": a, "finish": b}
            c.update(M.as_fixture(got))
            out["seeks"].append(c)
        # irregular lines: what the reference pops, how it ends and what it says, in a forked child
        out["irregular"] = []
        for name, (data, flags, where) in M.irregular_cases().items():
            if name.split(" / ")[0] in M.UNDEFINED_IN_REFERENCE:
                out["irregular"].append({"name": name, "flags": flags, "undefined": True})
                continue
            open(path, "wb").write(data)
            outpath = os.path.join(tmp, "out.txt")
            status, err = in_child(tmp, path, lambda: run_file(lib, path, 1 if flags & M.BED else 0, outpath))
            c = {"name": name, "flags": flags, "input_sha256": hashlib.sha256(data).hexdigest(), "exit_status": status, "stderr": err}
            c.update(M.as_fixture(parse(open(outpath, "rb").read())))
            out["irregular"].append(c)
    dst = os.path.join(HERE, "read_fixtures.json")
    with open(dst, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    size = os.path.getsize(dst)
    print("wrote %d readings, every one equal to the model record for record, %d bytes" % (len(out["cases"]), size))
    assert size < 400000, size


if __name__ == "__main__":
    main()
