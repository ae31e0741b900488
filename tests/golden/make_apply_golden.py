#!/usr/bin/env python
"""Generates tests/golden/apply_fixtures.json: small datasets and regions and the VERBATIM statistics of the compiled
reference's ApplyMultiplexer (src/apply.c; `apply`) over them -- AUC meanI varI stddevI CVI maxI minI per region, strict and
with fill-in.

The driver below is our own: two array-backed child iterators and a loop that pops the reference's Multiplexer to its end.
The array child implements seek as the reference's readers do (wigReader.c:192-215): it repositions to the first run that
ends after `start` and clips at `finish`.  It is compiled together with the reference's sources, unmodified and from where they
lie, into a shared object in a temporary directory (symbols the sources mention and this run never calls stay unresolved: the
object is loaded with lazy binding).  Nothing compiled is kept.

Cases: 1-3 chromosomes, a chromosome missing on either side; overlapping, nested and identical regions,
tests/golden/overlapping.bed among them; regions in gaps, before the first run and after the last; edges on run edges;
defaults 0, 1.5 and NaN; every region shorter than 10^6 bp; values k / 8 (exact in float32).  Cases with k % 5 == 4 put NaN
values into the dataset and record only AUC / meanI / maxI / minI: the reference's variance loop does not end on a NaN run
(nor, in fill-in mode, on a gap filled with a NaN default: those recordings hold the four statistics too).

Run where the reference's sources are present:  python tests/golden/make_apply_golden.py <path to the reference>
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
import region_model as RM  # noqa: E402
from make_coverage_golden import REF_SRCS, read_bed  # noqa: E402

STATS = ["AUC", "meanI", "varI", "stddevI", "CVI", "maxI", "minI"]
WITHOUT_VARIANCE = [0, 1, 5, 6]

DRIVER = r'''
#include <stdlib.h>
#include <string.h>
#include "wiggletools.h"
#include "wiggleIterator.h"
#include "multiplexer.h"

typedef struct {
    int n_chrom;
    char **names;
    long long *seg_off;
    int *start, *finish;
    double *value;
    int c;
    long long j;
    const char *stop_chrom;
    int stop;
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
    if (a->stop_chrom) {
        int cmp = strcmp(wi->chrom, a->stop_chrom);
        if (cmp > 0 || (cmp == 0 && wi->start >= a->stop)) wi->done = true;
        else if (cmp == 0 && wi->finish > a->stop) wi->finish = a->stop;
    }
}

static void arr_seek(WiggleIterator *wi, const char *chrom, int start, int finish) {
    ArrData *a = (ArrData *) wi->data;
    a->stop_chrom = chrom;
    a->stop = finish;
    a->c = 0;
    while (a->c < a->n_chrom && strcmp(a->names[a->c], chrom) < 0) a->c++;
    a->j = a->c < a->n_chrom ? a->seg_off[a->c] : a->seg_off[a->n_chrom];
    if (a->c < a->n_chrom && !strcmp(a->names[a->c], chrom)) {      /* the first run with finish > start (the runs do not overlap) */
        long long b0 = a->seg_off[a->c], b1 = a->seg_off[a->c + 1];
        while (b0 < b1) { long long mid = (b0 + b1) >> 1; if (a->finish[mid] > start) b1 = mid; else b0 = mid + 1; }
        a->j = b0;
    }
    wi->done = false;
    arr_pop(wi);
}

static WiggleIterator *arr_new(int n_chrom, char **names, long long *seg_off, int *start, int *finish, double *value, double default_value) {
    ArrData *a = (ArrData *) calloc(1, sizeof(ArrData));
    a->n_chrom = n_chrom; a->names = names; a->seg_off = seg_off; a->start = start; a->finish = finish; a->value = value;
    return newWiggleIterator(a, &arr_pop, &arr_seek, default_value, 0);
}

typedef WiggleIterator *(*StatFn)(WiggleIterator *);

/* stats: indices into {AUC, meanI, varI, stddevI, CVI, maxI, minI}.  Returns the number of regions the Multiplexer served. */
long long golden_apply(int n_chrom, char **names, long long *seg_off, int *start, int *finish, double *value, double default_value,
                       int r_chrom, char **r_names, long long *r_seg_off, int *r_start, int *r_finish, double *r_value,
                       int strict, int count, int *stats, long long cap, char **all_names, int n_all,
                       int *o_chrom, int *o_start, int *o_finish, double *o_values) {
    static StatFn all[7];
    StatFn fns[7];
    all[0] = AUCIntegrator; all[1] = MeanIntegrator; all[2] = VarianceIntegrator; all[3] = StandardDeviationIntegrator;
    all[4] = CoefficientOfVariationIntegrator; all[5] = MaxIntegrator; all[6] = MinIntegrator;
    for (int i = 0; i < count; i++) fns[i] = all[stats[i]];
    WiggleIterator *data = arr_new(n_chrom, names, seg_off, start, finish, value, default_value);
    WiggleIterator *regions = arr_new(r_chrom, r_names, r_seg_off, r_start, r_finish, r_value, 0);
    Multiplexer *m = ApplyMultiplexer(regions, fns, count, data, strict);
    long long n = 0;
    while (!m->done) {
        if (n < cap) {
            int c = 0;
            while (c < n_all && strcmp(all_names[c], m->chrom)) c++;
            o_chrom[n] = c; o_start[n] = m->start; o_finish[n] = m->finish;
            for (int i = 0; i < count; i++) o_values[n * count + i] = m->values[i];
        }
        n++;
        popMultiplexer(m);
    }
    return n;
}
'''


def build(ref, tmp):
    drv = os.path.join(tmp, "driver.c")
    open(drv, "w").write(DRIVER)
    so = os.path.join(tmp, "libapplygold.so")
    subprocess.check_call(["gcc", "-g", "-w", "-O3", "-std=gnu99", "-fPIC", "-shared", "-I" + os.path.join(ref, "src")] +
                          [os.path.join(ref, "src", s) for s in REF_SRCS + ["apply.c"]] + [drv, "-o", so, "-lm", "-lpthread"])
    return C.CDLL(so, mode=os.RTLD_LAZY)


def _side(names, per, value):
    arr = (C.c_char_p * max(len(names), 1))(*[x.encode() for x in names])
    seg = np.concatenate([[0], np.cumsum([len(p[0]) for p in per])]).astype(np.int64)
    s = np.concatenate([p[0] for p in per] + [np.zeros(0, np.int32)]).astype(np.int32)
    f = np.concatenate([p[1] for p in per] + [np.zeros(0, np.int32)]).astype(np.int32)
    v = np.ascontiguousarray(value, np.float64)
    return arr, seg, s, f, v


def run(L, all_names, data, regions, default, strict, stats):
    """data: (names, per-chromosome (start, finish), values); regions: (names, per-chromosome (start, finish))."""
    a, r = _side(*data), _side(regions[0], regions[1], np.ones(sum(len(p[0]) for p in regions[1])))
    cap = len(r[2]) + 8
    alln = (C.c_char_p * len(all_names))(*[x.encode() for x in all_names])
    st = np.array(stats, np.int32)
    oc, os_, of = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    ov = np.zeros((cap, len(stats)), np.float64)
    p = lambda x: C.c_void_p(x.ctypes.data)      # noqa: E731
    L.golden_apply.restype = C.c_longlong
    n = L.golden_apply(C.c_int(len(data[0])), a[0], p(a[1]), p(a[2]), p(a[3]), p(a[4]), C.c_double(default),
                       C.c_int(len(regions[0])), r[0], p(r[1]), p(r[2]), p(r[3]), p(r[4]),
                       C.c_int(int(strict)), C.c_int(len(stats)), p(st), C.c_longlong(cap), alln, C.c_int(len(all_names)),
                       p(oc), p(os_), p(of), p(ov))
    assert n == len(r[2]), (n, len(r[2]))
    num = lambda x: None if x != x else ("inf" if x == np.inf else "-inf" if x == -np.inf else x)      # noqa: E731
    rec = {"chrom": oc[:n].tolist(), "start": os_[:n].tolist(), "finish": of[:n].tolist()}
    for i, k in enumerate(stats):
        rec[STATS[k]] = [num(x) for x in ov[:n, i].tolist()]
    return rec


def regions_for(rng, k, d, span, first=True):
    """Regions sorted by start over one chromosome whose dataset is d: overlapping, nested, identical, in gaps, before the first
    run and after the last, with edges on run edges."""
    s, f = d
    n = int(rng.integers(1, 3))
    rs, rf = (x.astype(np.int64) for x in CM.random_segment(rng, n, span, max(2, span // int(rng.choice([2, 6, 20])))))
    extra = []
    if len(s) and first:                                            # two kinds per case, by turns, on its first chromosome (the file stays small)
        i = int(rng.integers(0, len(s)))
        j = int(rng.integers(i, len(s)))
        if k % 4 == 0:
            extra.append((int(s[i]), int(f[j])))                    # edges on run edges
            extra.append((int(f[i]), int(f[i]) + 1 + int(rng.integers(0, 4))))   # from a run's end on: a gap, or the next run
        elif k % 4 == 1:
            extra.append((int(s[i]), int(f[j])))                    # identical, and
            extra.append((int(s[i]), int(f[j])))
            extra.append((max(int(s[0]) - 2, 0), int(f[-1]) + 2))   # around everything: the others nest in it
        elif k % 4 == 2:
            extra.append((max(int(s[0]) - 5, 0), max(int(s[0]) - 1, 1)))    # before the first run
            extra.append((int(f[-1]), int(f[-1]) + 7))              # after the last, touching it
        else:
            extra.append((int(s[i]) + (1 if s[i] + 1 < f[i] - 1 else 0), int(f[i]) - (1 if s[i] + 1 < f[i] - 1 else 0)))    # inside one run
            extra.append((int(s[i]), int(f[j]) + 3))                # a nest for it, ending in a gap or the next run
    if extra:
        rs = np.concatenate([rs, [e[0] for e in extra]])
        rf = np.concatenate([rf, [e[1] for e in extra]])
    rf = np.maximum(rf, rs + 1)
    o = np.argsort(rs, kind="stable")
    return rs[o].astype(np.int32), rf[o].astype(np.int32)


def main():
    ref = sys.argv[1]
    rng = np.random.default_rng(20261020)
    all_names = ["chr1", "chr2", "chr3"]
    cases = []
    bed_names, bed = read_bed(os.path.join(HERE, "overlapping.bed"))
    for k in range(150):
        span = int((30, 200, 3000)[k % 3])
        present_d = [c for c in range(3) if c < 1 + k % 3]
        present_r = list(present_d)
        if k % 7 == 3 and len(present_d) > 1:
            present_d = present_d[1:]                   # a chromosome only the regions have
        if k % 7 == 5 and len(present_r) > 1:
            present_r = present_r[:-1]                  # ... and one only the dataset has
        if k % 11 == 6:
            present_r = [0, 2]
        n_max = 20 if k % 10 == 0 else 9
        data = [RM.disjoint_segment(rng, int(rng.integers(1, n_max)), span) for _ in present_d]
        if k < 4:
            names_r = bed_names
            regs = [(np.array([iv[0] for iv in p], np.int32), np.array([iv[1] for iv in p], np.int32)) for p in bed]
            names_d = bed_names[:len(present_d)]
            data = data[:len(names_d)]
            local_all = sorted(set(bed_names))
        else:
            names_d = [all_names[c] for c in present_d]
            names_r = [all_names[c] for c in present_r]
            by_name = dict(zip(names_d, data))
            empty = (np.zeros(0, np.int32), np.zeros(0, np.int32))
            regs = [regions_for(rng, k, by_name.get(nm, empty), span, q == 0 or nm not in by_name) for q, nm in enumerate(names_r)]
            local_all = all_names
        n_d = sum(len(p[0]) for p in data)
        value = rng.integers(-80, 80, n_d) / 8.0                # exact in float32
        with_nan = k % 5 == 4
        if with_nan:
            value[rng.random(n_d) < 0.3] = np.nan
        default = (0.0, 1.5, float("nan"))[(k // 2) % 3]
        cases.append(("case%03d" % k, local_all, (names_d, data, value), (names_r, regs), default, with_nan))
    out = {"generator": "tests/golden/make_apply_golden.py",
           "source": "compiled reference v1.2.11: ApplyMultiplexer over array-backed children, statistics in the order of `stats`",
           "stats": STATS, "cases": []}
    with tempfile.TemporaryDirectory() as tmp:
        L = build(ref, tmp)
        for name, local_all, data, regs, default, with_nan in cases:
            rec = {"name": name, "chrom_names": local_all, "default": None if default != default else default, "nan_values": with_nan}
            d, r = _side(*data), _side(regs[0], regs[1], np.zeros(0))
            rec["data"] = {"chroms": [local_all.index(x) for x in data[0]], "seg_off": d[1].tolist(), "start": d[2].tolist(), "finish": d[3].tolist(),
                           "value": [None if x != x else x for x in d[4].tolist()]}
            rec["regions"] = {"chroms": [local_all.index(x) for x in regs[0]], "seg_off": r[1].tolist(), "start": r[2].tolist(), "finish": r[3].tolist()}
            stats = WITHOUT_VARIANCE if with_nan else list(range(7))
            rec["strict"] = run(L, local_all, data, regs, default, True, stats)
            # (a NaN default fills the gaps with NaN runs: the same loop that does not end)
            rec["fillin"] = run(L, local_all, data, regs, default, False, WITHOUT_VARIANCE if default != default else stats)
            out["cases"].append(rec)
    path = os.path.join(HERE, "apply_fixtures.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    print("wrote %d cases, %d bytes" % (len(out["cases"]), os.path.getsize(path)))


if __name__ == "__main__":
    main()
