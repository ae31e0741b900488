#!/usr/bin/env python
"""Generates tests/golden/coverage_fixtures.json: small overlapping inputs and the VERBATIM output of the compiled reference's
CoverageWiggleIterator (src/unaryOps.c:303-375) and UnionWiggleIterator (:60-92) over them.

The driver below is our own: an array-backed child iterator with `overlaps = true` and a loop that pops the reference's
iterator to its end.  It is compiled together with the reference's sources, unmodified and from where they lie, into a
shared object in a temporary directory (the reader symbols unaryOps.c mentions stay unresolved: the object is loaded with
lazy binding and they are never called).  Nothing compiled is kept.

The reference's coverage output contains one run with start == finish per non-empty stream (it reads the exhausted child's
stale start, :333-334); it is recorded as it comes and stripped by the tests (tests/cover_model.py).

Run where the reference's sources are present:  python tests/golden/make_coverage_golden.py [path to the reference]
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cover_model as M  # noqa: E402

REF_SRCS = ["wiggleIterator.c", "multiplexer.c", "multiSet.c", "reducers.c", "fib.c", "recycleBin.c", "unaryOps.c", "statistics.c",
            "wigReader.c", "bedReader.c", "bufferedReader.c", "samReader.c", "vcfReader.c", "hash.c", "hashfib.c", "wigWriter.c",
            "mWigWriter.c"]

DRIVER = r'''
#include <stdlib.h>
#include <string.h>
#include "wiggletools.h"
#include "wiggleIterator.h"

typedef struct {
    int n_chrom;
    char **names;
    long long *seg_off;
    int *start, *finish;
    double *value;
    int c;
    long long j;
} ArrData;

static void arr_pop(WiggleIterator *wi) {
    ArrData *a = (ArrData *) wi->data;
    while (a->c < a->n_chrom && a->j >= a->seg_off[a->c + 1]) a->c++;
    if (a->c >= a->n_chrom) { wi->done = true; return; }
    wi->chrom = a->names[a->c];
    wi->start = a->start[a->j];
    wi->finish = a->finish[a->j];
    wi->value = a->value[a->j];
    a->j++;
}

static void arr_seek(WiggleIterator *wi, const char *chrom, int start, int finish) { }

/* which: 0 coverage, 1 union.  Returns the number of elements the reference's iterator delivered. */
long long golden_run(int which, int n_chrom, char **names, long long *seg_off, int *start, int *finish, double *value,
                     long long cap, int *o_chrom, int *o_start, int *o_finish, double *o_value) {
    ArrData *a = (ArrData *) calloc(1, sizeof(ArrData));
    a->n_chrom = n_chrom; a->names = names; a->seg_off = seg_off; a->start = start; a->finish = finish; a->value = value;
    WiggleIterator *child = newWiggleIterator(a, &arr_pop, &arr_seek, 0, true);
    WiggleIterator *wi = which == 0 ? CoverageWiggleIterator(child) : UnionWiggleIterator(child);
    long long n = 0;
    while (!wi->done) {
        if (n < cap) {
            int c = 0;
            while (c < n_chrom && strcmp(names[c], wi->chrom)) c++;
            o_chrom[n] = c; o_start[n] = wi->start; o_finish[n] = wi->finish; o_value[n] = wi->value;
        }
        n++;
        pop(wi);
    }
    return n;
}
'''


def build(ref, tmp):
    drv = os.path.join(tmp, "driver.c")
    open(drv, "w").write(DRIVER)
    so = os.path.join(tmp, "libcovgold.so")
    subprocess.check_call(["gcc", "-g", "-w", "-O3", "-std=gnu99", "-fPIC", "-shared", "-I" + os.path.join(ref, "src")] +
                          [os.path.join(ref, "src", s) for s in REF_SRCS] + [drv, "-o", so, "-lm", "-lpthread"])
    return C.CDLL(so, mode=os.RTLD_LAZY)


def run(L, which, names, seg_off, start, finish, value):
    n = len(start)
    cap = 2 * n + 8
    arr = (C.c_char_p * len(names))(*[x.encode() for x in names])
    seg = np.ascontiguousarray(seg_off, np.int64)
    s, f, v = np.ascontiguousarray(start, np.int32), np.ascontiguousarray(finish, np.int32), np.ascontiguousarray(value, np.float64)
    oc, os_, of, ov = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.float64)
    L.golden_run.restype = C.c_longlong
    m = L.golden_run(C.c_int(which), C.c_int(len(names)), arr, C.c_void_p(seg.ctypes.data), C.c_void_p(s.ctypes.data), C.c_void_p(f.ctypes.data),
                     C.c_void_p(v.ctypes.data), C.c_longlong(cap), C.c_void_p(oc.ctypes.data), C.c_void_p(os_.ctypes.data),
                     C.c_void_p(of.ctypes.data), C.c_void_p(ov.ctypes.data))
    assert m <= cap, (m, cap)
    return {"chrom": oc[:m].tolist(), "start": os_[:m].tolist(), "finish": of[:m].tolist(), "value": ov[:m].tolist()}


def read_bed(path):
    """Columns 2 and 3 of a BED file as [start, finish) per chromosome, in file order (the reference's reader shifts both by
    one, bedReader.c:43-44, which moves the depth track and changes nothing else)."""
    rows = {}
    for line in open(path):
        p = line.split()
        if len(p) >= 3:
            rows.setdefault(p[0], []).append((int(p[1]), int(p[2])))
    names = sorted(rows)
    return names, [rows[n] for n in names]


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    rng = np.random.default_rng(20261018)
    cases = []
    names, per = read_bed(os.path.join(HERE, "overlapping.bed"))
    cases.append(("overlapping.bed", names, per, None))
    for k in range(200):
        n_chrom = int(rng.integers(1, 4))
        span = int((20, 200, 5000)[k % 3])
        per = []
        for _ in range(n_chrom):
            n = int(rng.integers(1, 60 if k % 10 == 0 else (8 if k % 4 == 0 else 18)))
            s, f = M.random_segment(rng, n, span, max(2, span // int(rng.choice([2, 8, 40]))))
            per.append(list(zip(s.tolist(), f.tolist())))
        cases.append(("random%03d" % k, ["chr%d" % (c + 1) for c in range(n_chrom)], per, rng))
    out = {"generator": "tests/golden/make_coverage_golden.py",
           "source": "compiled reference v1.2.11: CoverageWiggleIterator / UnionWiggleIterator over an array-backed child with overlaps = true",
           "cases": []}
    with tempfile.TemporaryDirectory() as tmp:
        L = build(ref, tmp)
        for name, names, per, r in cases:
            seg_off = np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.int64)
            start = np.array([iv[0] for p in per for iv in p], np.int32)
            finish = np.array([iv[1] for p in per for iv in p], np.int32)
            # values exact in float32 (k / 8), so the union's value survives every route bit for bit
            value = np.ones(len(start)) if r is None else r.integers(-80, 80, len(start)) / 8.0
            out["cases"].append({"name": name, "chrom_names": names, "seg_off": seg_off.tolist(), "start": start.tolist(),
                                 "finish": finish.tolist(), "value": value.tolist(),
                                 "coverage": run(L, 0, names, seg_off, start, finish, value),
                                 "union": run(L, 1, names, seg_off, start, finish, value)})
    path = os.path.join(HERE, "coverage_fixtures.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    print("wrote %d cases, %d bytes" % (len(out["cases"]), os.path.getsize(path)))


if __name__ == "__main__":
    main()
