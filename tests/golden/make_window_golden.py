#!/usr/bin/env python
"""Generates tests/golden/window_fixtures.json: small run lists and the VERBATIM output of the compiled reference's
BinningWiggleIterator and SmoothWiggleIterator (src/unaryOps.c:963-1162; `bin`, `smooth`) over them, pop by pop.

The driver is our own: the array-backed child iterator of make_apply_golden.py and a loop that pops the reference's iterator
to its end, optionally after one pop and a seek.  It is compiled together with the reference's sources, unmodified and from
where they lie, into a shared object in a temporary directory.  Nothing compiled is kept.

Cases: 1-3 chromosomes with spans 30 / 200 / 3000 bp; values k / 8, NaN runs in every fifth case; defaults cycling 0, NaN, 1.5;
widths cycling 2, 3, 7, 10, 64, 100 (h = width / 2); first starts cycling 1, h, h + 1 and far above; in every case with more than
one chromosome the second one is shorter than the width and, where h > 1, a third one is shorter than h; gaps of width - 1,
width and width + 1 among the random ones; runs that end exactly on a bin edge; every tenth case also records a seek for both
operators.  Smooth output is stored run-length encoded per island (window_model.recorded).

All values are multiples of 1/8 below 2^20 in size, so every sum the reference forms is exact whatever its order, and a value
is that sum (bin) or one correctly rounded quotient of it (smooth): the generator asserts that the Fraction model of
tests/window_model.py gives every recorded value bit for bit -- none is left out of the comparison.

Run where the reference's sources are present:  python tests/golden/make_window_golden.py <path to the reference>
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
import make_apply_golden as AG  # noqa: E402
import window_model as M  # noqa: E402
from make_coverage_golden import REF_SRCS  # noqa: E402

DRIVER = AG.DRIVER + r'''
/* op 0: bin, 1: smooth.  seek_chrom >= 0: one pop, then seek(names[seek_chrom], lo, hi).  Returns the number of pops served. */
long long golden_window(int op, int n_chrom, char **names, long long *seg_off, int *start, int *finish, double *value, double default_value,
                        int width, int seek_chrom, int lo, int hi, long long cap, int *o_chrom, int *o_start, int *o_finish, double *o_value) {
    WiggleIterator *child = arr_new(n_chrom, names, seg_off, start, finish, value, default_value);
    WiggleIterator *wi = op ? SmoothWiggleIterator(child, width) : BinningWiggleIterator(child, width);
    long long n = 0;
    if (seek_chrom >= 0) {
        pop(wi);
        seek(wi, names[seek_chrom], lo, hi);
    }
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
double golden_default(int op, double default_value, int width) {
    int s = 1, f = 2; long long seg[2] = {0, 1}; double v = 0; char *names[1] = {"chr1"};
    WiggleIterator *child = arr_new(1, names, seg, &s, &f, &v, default_value);
    return (op ? SmoothWiggleIterator(child, width) : BinningWiggleIterator(child, width))->default_value;
}
'''


def build(ref, tmp):
    drv = os.path.join(tmp, "driver.c")
    open(drv, "w").write(DRIVER)
    so = os.path.join(tmp, "libwindowgold.so")
    subprocess.check_call(["gcc", "-g", "-w", "-O3", "-std=gnu99", "-fPIC", "-shared", "-I" + os.path.join(ref, "src")] +
                          [os.path.join(ref, "src", s) for s in REF_SRCS] + [drv, "-o", so, "-lm", "-lpthread"])
    return C.CDLL(so, mode=os.RTLD_LAZY)


def run(L, op, names, case, default, width, seek=None):
    cap = M.smooth_capacity(case, width) + M.bin_capacity(case, width) + 8
    arr = (C.c_char_p * len(names))(*[x.encode() for x in names])
    oc, os_, of, ov = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.float64)
    p = lambda x: C.c_void_p(x.ctypes.data)      # noqa: E731
    sk = seek or (-1, 0, 0)
    L.golden_window.restype = C.c_longlong
    n = L.golden_window(C.c_int(op), C.c_int(len(names)), arr, p(case.seg), p(case.s), p(case.f), p(case.v), C.c_double(default), C.c_int(width),
                        C.c_int(sk[0]), C.c_int(sk[1]), C.c_int(sk[2]), C.c_longlong(cap), p(oc), p(os_), p(of), p(ov))
    assert 0 <= n <= cap, (n, cap)
    return [(int(c), int(a), int(b), float(x)) for c, a, b, x in zip(oc[:n], os_[:n], of[:n], ov[:n])]


def num(x):
    return None if x != x else x


def store(op, rows):
    if op == 0:
        return {"rows": [[c, a, b, num(x)] for c, a, b, x in rows]}
    islands, nxt = [], None           # [chromosome, first position, [[value, count]]]
    for c, a, b, x in rows:
        assert b == a + 1
        if not islands or islands[-1][0] != c or nxt != a:
            islands.append([c, a, []])
        vals = islands[-1][2]
        if vals and (np.float64(vals[-1][0]).tobytes() == np.float64(x).tobytes() or (vals[-1][0] != vals[-1][0] and x != x)):
            vals[-1][1] += 1
        else:
            vals.append([x, 1])
        nxt = a + 1
    return {"islands": [[c, a, [num(v) if n == 1 else [num(v), n] for v, n in vals]] for c, a, vals in islands]}


def make_case(rng, k):
    span = int((30, 200, 3000)[k % 3])
    w = M.WIDTHS[k % len(M.WIDTHS)]
    h = w // 2
    n_chrom = 1 + (k // 3) % 3
    first = (1, max(h, 1), h + 1, 3 * w + 11)[(k // 2) % 4]
    gaps = (0, 0, 1, 2, w - 1, w, w + 1, int(rng.integers(1, max(span // 8, 2))))
    lengths = (1, 2, 3, w - 1, w, w + 1, int(rng.integers(1, max(span // 8, 2))))
    s, f, v = M.runs_from(rng, first, 60, lengths, gaps)
    edge = 1 + ((f - 1 + w - 1) // w) * w                             # every third run ends exactly on a bin edge where that fits
    for i in range(0, len(s), 3):
        if i + 1 >= len(s) or edge[i] <= s[i + 1]:
            f[i] = edge[i]
    keep = s < first + span
    keep[0] = True
    chroms = [(s[keep][:16], f[keep][:16], v[keep][:16])]
    if n_chrom >= 2:                                                  # a chromosome shorter than the width
        ln = int(rng.integers(1, w))
        a = int(rng.integers(1, 2 * w))
        chroms.append(([a, a + max(ln // 2, 1)][:1 + (ln > 1)], [a + max(ln // 2, 1), a + ln][:1 + (ln > 1)], (rng.integers(-80, 80, 2) / 8.0)[:1 + (ln > 1)]))
    if n_chrom >= 3:                                                  # ... and one shorter than h (where h > 1), next to the start
        ln = int(rng.integers(1, max(h, 2)))
        a = (1, max(h - ln, 1), h + 1)[k % 3]
        chroms.append(([a], [a + ln], [rng.integers(-80, 80) / 8.0]))
    case = M.Case(chroms)
    if k % 5 == 4:
        v = case.chroms[0][2]
        v[rng.random(len(v)) < 0.3] = np.nan
        v[0] = np.nan
        case = M.Case(case.chroms)
    return case, w


def main():
    ref = sys.argv[1]
    rng = np.random.default_rng(20261022)
    all_names = ["chr1", "chr2", "chr3"]
    out = {"generator": "tests/golden/make_window_golden.py",
           "source": "compiled reference v1.2.11: BinningWiggleIterator and SmoothWiggleIterator over an array-backed child, every pop",
           "cases": []}
    compared = 0
    seeks = [0, 0]
    with tempfile.TemporaryDirectory() as tmp:
        L = build(ref, tmp)
        L.golden_default.restype = C.c_double
        for k in range(60):
            case, w = make_case(rng, k)
            default = M.DEFAULTS[(k // 2) % 3]
            names = all_names[:len(case.chroms)]
            rec = {"name": "case%03d" % k, "chrom_names": names, "default": num(default), "width": w, "seg_off": case.seg.tolist(),
                   "start": case.s.tolist(), "finish": case.f.tolist(), "value": [num(x) for x in case.v.tolist()]}
            assert all(x != x or (x * 8 == int(x * 8) and abs(x) < 2 ** 20) for x in case.v.tolist() + [default])
            for op, name in ((0, "bin"), (1, "smooth")):
                rows = run(L, op, names, case, default, w)
                model = M.bin(case.chroms, w, default) if op == 0 else M.smooth(case.chroms, w)
                assert [r[:3] for r in rows] == [r[:3] for r in model], (k, name)
                assert M.same_bits([r[3] for r in rows], [r[3].float() for r in model]), (k, name)
                compared += len(rows)
                if op == 0:
                    assert all((r[1] - 1) % w == 0 and r[2] == r[1] + w for r in rows), (k, "grid")
                rec[name] = store(op, rows)
                back = M.recorded(rec[name])
                assert [r[:3] for r in back] == [r[:3] for r in rows] and M.same_bits([r[3] for r in back], [r[3] for r in rows]), (k, name, "stored")
                d = L.golden_default(C.c_int(op), C.c_double(default), C.c_int(w))
                rec[name]["default"] = num(d)
                if k % 10 == 0:
                    g = len(case.chroms) - 1 if k % 20 else 0
                    s, f, _ = case.chroms[g]
                    lo, hi = int(s[0]) + 1, int(f[-1]) - 1
                    if hi > lo:
                        rows = run(L, op, names, case, default, w, (g, lo, hi))
                        sub = M.seek_child(case, g, lo, hi)
                        model = M.bin(sub.chroms, w, default) if op == 0 else M.smooth(sub.chroms, w)
                        assert [r[:3] for r in rows] == [r[:3] for r in model], (k, name, "seek")
                        assert M.same_bits([r[3] for r in rows], [r[3].float() for r in model]), (k, name, "seek")
                        compared += len(rows)
                        rec[name]["seek"] = dict(store(op, rows), chrom=g, lo=lo, hi=hi)
                        seeks[op] += 1
            out["cases"].append(rec)
    assert min(seeks) >= 1, seeks
    path = os.path.join(HERE, "window_fixtures.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    size = os.path.getsize(path)
    print("wrote %d cases, %d recorded values all equal to the model bit for bit, %d seeks, %d bytes" % (len(out["cases"]), compared, sum(seeks), size))
    assert size < 250000, size


if __name__ == "__main__":
    main()
