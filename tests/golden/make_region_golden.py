#!/usr/bin/env python
"""Generates tests/golden/region_fixtures.json: small sources and masks and the VERBATIM output of the compiled reference's
OverlapWiggleIterator, NoverlapWiggleIterator, TrimWiggleIterator and NearestWiggleIterator (src/unaryOps.c:437-639) over
them.

The driver below is our own: two array-backed child iterators (the `overlaps` flag of each as the case says) and a loop that
pops the reference's iterator to its end.  It is compiled together with the reference's sources, unmodified and from where
they lie, into a shared object in a temporary directory (the reader symbols unaryOps.c mentions stay unresolved: the object
is loaded with lazy binding and they are never called).  Nothing compiled is kept.

Cases: the four operators over 1-3 chromosomes, a chromosome missing on either side, sources that overlap themselves (for a
trim these are recorded under "trim_overlapping_source": the reference's output then depends on its pop order and is not what
the device door computes, which refuses such a source), and tests/golden/overlapping.bed as the mask.

Run where the reference's sources are present:  python tests/golden/make_region_golden.py <path to the reference>
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
import cover_model as CM  # noqa: E402
import region_model as M  # noqa: E402
from make_coverage_golden import REF_SRCS, read_bed  # noqa: E402

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

static WiggleIterator *arr_new(int n_chrom, char **names, long long *seg_off, int *start, int *finish, double *value, int overlaps) {
    ArrData *a = (ArrData *) calloc(1, sizeof(ArrData));
    a->n_chrom = n_chrom; a->names = names; a->seg_off = seg_off; a->start = start; a->finish = finish; a->value = value;
    return newWiggleIterator(a, &arr_pop, &arr_seek, 0, overlaps);
}

/* op: 0 overlaps, 1 noverlaps, 2 trim, 3 nearest.  Returns the number of elements the reference's iterator delivered. */
long long golden_region(int op, int n_chrom, char **names, long long *seg_off, int *start, int *finish, double *value, int overlaps,
                        int m_chrom, char **m_names, long long *m_seg_off, int *m_start, int *m_finish, double *m_value, int m_overlaps,
                        long long cap, char **all_names, int n_all, int *o_chrom, int *o_start, int *o_finish, double *o_value) {
    WiggleIterator *src = arr_new(n_chrom, names, seg_off, start, finish, value, overlaps);
    WiggleIterator *mask = arr_new(m_chrom, m_names, m_seg_off, m_start, m_finish, m_value, m_overlaps);
    WiggleIterator *wi = op == 0 ? OverlapWiggleIterator(src, mask) : op == 1 ? NoverlapWiggleIterator(src, mask)
                       : op == 2 ? TrimWiggleIterator(src, mask) : NearestWiggleIterator(src, mask);
    long long n = 0;
    while (!wi->done) {
        if (n < cap) {
            int c = 0;
            while (c < n_all && strcmp(all_names[c], wi->chrom)) c++;
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
    so = os.path.join(tmp, "libreggold.so")
    subprocess.check_call(["gcc", "-g", "-w", "-O3", "-std=gnu99", "-fPIC", "-shared", "-I" + os.path.join(ref, "src")] +
                          [os.path.join(ref, "src", s) for s in REF_SRCS] + [drv, "-o", so, "-lm", "-lpthread"])
    return C.CDLL(so, mode=os.RTLD_LAZY)


def _side(names, per, value):
    arr = (C.c_char_p * max(len(names), 1))(*[x.encode() for x in names])
    seg = np.concatenate([[0], np.cumsum([len(p[0]) for p in per])]).astype(np.int64)
    s = np.concatenate([p[0] for p in per] + [np.zeros(0, np.int32)]).astype(np.int32)
    f = np.concatenate([p[1] for p in per] + [np.zeros(0, np.int32)]).astype(np.int32)
    v = np.ascontiguousarray(value, np.float64)
    return arr, seg, s, f, v


def run(L, op, all_names, src, mask):
    """src / mask: (names, per-chromosome (start, finish), values, overlaps flag)."""
    a, m = _side(*src[:3]), _side(*mask[:3])
    cap = len(a[2]) + len(m[2]) + 8
    alln = (C.c_char_p * len(all_names))(*[x.encode() for x in all_names])
    oc, os_, of, ov = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.float64)
    p = lambda x: C.c_void_p(x.ctypes.data)      # noqa: E731
    L.golden_region.restype = C.c_longlong
    n = L.golden_region(C.c_int(op), C.c_int(len(src[0])), a[0], p(a[1]), p(a[2]), p(a[3]), p(a[4]), C.c_int(int(src[3])),
                        C.c_int(len(mask[0])), m[0], p(m[1]), p(m[2]), p(m[3]), p(m[4]), C.c_int(int(mask[3])),
                        C.c_longlong(cap), alln, C.c_int(len(all_names)), p(oc), p(os_), p(of), p(ov))
    assert n <= cap, (n, cap)
    # (NaN: nearest without a candidate) as null
    return {"chrom": oc[:n].tolist(), "start": os_[:n].tolist(), "finish": of[:n].tolist(),
            "value": [None if x != x else x for x in ov[:n].tolist()]}


def main():
    ref = sys.argv[1]
    rng = np.random.default_rng(20261019)
    all_names = ["chr1", "chr2", "chr3"]
    cases = []
    bed_names, bed = read_bed(os.path.join(HERE, "overlapping.bed"))
    for k in range(150):
        span = int((30, 200, 3000)[k % 3])
        present_s = [c for c in range(3) if c < 1 + k % 3]
        present_m = list(present_s)
        if k % 7 == 3 and len(present_s) > 1:
            present_s = present_s[1:]                   # a chromosome only the mask has
        if k % 7 == 5 and len(present_m) > 1:
            present_m = present_m[:-1]                  # ... and one only the source has
        if k % 11 == 6:
            present_m = [0, 2]
        overlapping_source = k % 3 == 1
        n_max = 40 if k % 10 == 0 else 12
        src = []
        for _ in present_s:
            n = int(rng.integers(1, n_max))
            src.append(CM.random_segment(rng, n, span, max(2, span // 6)) if overlapping_source else M.disjoint_segment(rng, n, span))
        if k < 4:
            mask_names, mask = bed_names, [(np.array([iv[0] for iv in p], np.int32), np.array([iv[1] for iv in p], np.int32)) for p in bed]
            names_s = bed_names[:len(present_s)] if len(bed_names) >= len(present_s) else bed_names
            src = src[:len(names_s)]
            local_all = sorted(set(bed_names))
        else:
            mask_names = [all_names[c] for c in present_m]
            mask = [CM.random_segment(rng, int(rng.integers(1, n_max)), span, max(2, span // int(rng.choice([3, 10, 30])))) for _ in present_m]
            names_s = [all_names[c] for c in present_s]
            local_all = all_names
        n_src = sum(len(p[0]) for p in src)
        value = rng.integers(-80, 80, n_src) / 8.0         # exact in float32
        cases.append(("case%03d" % k, local_all, (names_s, src, value, overlapping_source),
                      (mask_names, mask, np.ones(sum(len(p[0]) for p in mask)), True)))
    out = {"generator": "tests/golden/make_region_golden.py",
           "source": "compiled reference v1.2.11: Overlap / Noverlap / Trim / NearestWiggleIterator over array-backed children",
           "cases": []}
    with tempfile.TemporaryDirectory() as tmp:
        L = build(ref, tmp)
        for name, local_all, src, mask in cases:
            rec = {"name": name, "chrom_names": local_all}
            for tag, side in (("source", src), ("mask", mask)):
                rec[tag] = {"chroms": [local_all.index(x) for x in side[0]], "seg_off": _side(*side[:3])[1].tolist(),
                            "start": _side(*side[:3])[2].tolist(), "finish": _side(*side[:3])[3].tolist()}
            rec["source"]["value"] = src[2].tolist()
            rec["source"]["overlaps"] = bool(src[3])
            for op_name, op in M.OPS.items():
                key = "trim_overlapping_source" if op_name == "trim" and src[3] else op_name
                rec[key] = run(L, op, local_all, src, mask)
            out["cases"].append(rec)
    path = os.path.join(HERE, "region_fixtures.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    print("wrote %d cases, %d bytes" % (len(out["cases"]), os.path.getsize(path)))


if __name__ == "__main__":
    main()
