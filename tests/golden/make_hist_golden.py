#!/usr/bin/env python
"""Generates tests/golden/hist_fixtures.json: small run lists and the VERBATIM output of the compiled reference's histogram(),
print_histogram() and normalize_histogram() + print_histogram() (src/plots.c:167-223; `histogram`) over them.

The driver is our own: the array-backed child iterator of make_apply_golden.py, one per row, and a function that calls the
three entry points and copies the matrix, the range and the two texts out.  It is compiled together with the reference's
sources, unmodified and from where they lie, into a shared object in a temporary directory.  Nothing compiled is kept.

Cases: widths cycling 1, 2, 3, 7, 10, 64, 100; 1-3 rows of at most 40 runs, a later row sometimes empty or all NaN; values
alternately multiples of 1/8 and full-mantissa doubles; NaN runs in every fifth case, in one of them leading row 0; runs that
overlap and are not sorted in two cases of three; cases with all values equal; values exactly equal to the maximum; one column
past 2^32 (five runs of length 2^30).  The two extremes come first in row 0 -- low then high and high then low by turns at
width >= 2, low then high at width 1 --, which is the condition (hist_model.reference_equal) under which the reference's
streaming histogram never re-bins a run it has placed and so equals the exact two-pass rule.  The generator asserts that
condition and that the reference's matrix and range equal tests/hist_model.py bit for bit, for every case: none is left out.

Run where the reference's sources are present:  python tests/golden/make_hist_golden.py <path to the reference>
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
import hist_model as M  # noqa: E402
import make_apply_golden as AG  # noqa: E402
from make_coverage_golden import REF_SRCS  # noqa: E402

DRIVER = AG.DRIVER + r'''
#include <stdio.h>

/* what plots.c keeps behind the opaque Histogram */
typedef struct { int width; int count; double **values; double min; double max; } HistView;

static long long text_of(Histogram *h, char *out, long long cap) {
    char *buf = NULL;
    size_t len = 0;
    FILE *fp = open_memstream(&buf, &len);
    print_histogram(h, fp);
    fclose(fp);
    if ((long long) len < cap) { memcpy(out, buf, len); out[len] = 0; }
    free(buf);
    return (long long) len;
}

/* row r: the runs [row_off[r], row_off[r + 1]) as one chromosome.  Returns the longer text's length (above cap: too small). */
long long golden_hist(int n_rows, long long *row_off, int *start, int *finish, double *value, int width,
                      double *o_hist, double *o_range, long long cap, char *o_text, char *o_norm_text) {
    static char *names[1] = {"chr1"};
    WiggleIterator **wigs = (WiggleIterator **) calloc(n_rows, sizeof(WiggleIterator *));
    long long *seg = (long long *) calloc(2 * n_rows, sizeof(long long));
    for (int r = 0; r < n_rows; r++) {
        seg[2 * r] = 0; seg[2 * r + 1] = row_off[r + 1] - row_off[r];
        wigs[r] = arr_new(1, names, seg + 2 * r, start + row_off[r], finish + row_off[r], value + row_off[r], 0);
    }
    Histogram *h = histogram(wigs, n_rows, width);
    HistView *hv = (HistView *) h;
    for (int r = 0; r < n_rows; r++) for (int c = 0; c < width; c++) o_hist[(long long) r * width + c] = hv->values[r][c];
    o_range[0] = hv->min; o_range[1] = hv->max;
    long long a = text_of(h, o_text, cap);
    normalize_histogram(h);
    long long b = text_of(h, o_norm_text, cap);
    return a > b ? a : b;
}
'''


def build(ref, tmp):
    drv = os.path.join(tmp, "driver.c")
    open(drv, "w").write(DRIVER)
    so = os.path.join(tmp, "libhistgold.so")
    subprocess.check_call(["gcc", "-g", "-w", "-O3", "-std=gnu99", "-D_GNU_SOURCE", "-fPIC", "-shared", "-I" + os.path.join(ref, "src")] +
                          [os.path.join(ref, "src", s) for s in REF_SRCS + ["plots.c"]] + [drv, "-o", so, "-lm", "-lpthread"])
    return C.CDLL(so, mode=os.RTLD_LAZY)


def run(L, lists, width):
    cap = 1 << 16
    n_rows = lists.n_rows
    hist, rng = np.zeros((n_rows, width), np.float64), np.zeros(2, np.float64)
    t0, t1 = C.create_string_buffer(cap), C.create_string_buffer(cap)
    p = lambda x: C.c_void_p(x.ctypes.data)      # noqa: E731
    L.golden_hist.restype = C.c_longlong
    n = L.golden_hist(C.c_int(n_rows), p(lists.seg), p(lists.s), p(lists.f), p(lists.v), C.c_int(width), p(hist), p(rng), C.c_longlong(cap), t0, t1)
    assert 0 < n < cap, n
    return hist, rng, t0.value.decode(), t1.value.decode()


def make_case(rng, k):
    w = M.WIDTHS[k % len(M.WIDTHS)]
    n_rows = 1 + k % 3
    eighths = k % 2 == 0
    draw = (lambda n: rng.integers(-80, 81, n) / 8.0) if eighths else (lambda n: rng.uniform(-10, 10, n))
    rows = []
    for r in range(n_rows):
        n = int(rng.integers(4, 41 if k % 10 == 0 else 20))
        if k % 3 == 0:                                      # sorted and disjoint
            ln = rng.integers(1, 30, n)
            s = 1 + np.cumsum(rng.integers(0, 9, n) + np.concatenate([[0], ln[:-1]]))
        else:                                               # neither
            s, ln = rng.integers(1, 300, n), rng.integers(1, 60, n)
        rows.append([s.astype(np.int32), (s + ln).astype(np.int32), draw(n)])
    if k % 15 == 7:
        for r in rows:
            r[2][:] = rows[0][2][0]
    allv = np.concatenate([r[2] for r in rows])
    lo, hi = allv.min(), allv.max()
    if lo < hi:                                             # the two extremes first in row 0
        low_high = w == 1 or (k // 7) % 2 == 0
        rows[0][2][:2] = (lo, hi) if low_high else (hi, lo)
        for r in rows:                                      # values exactly equal to the maximum
            if len(r[2]) > 3:
                r[2][3] = hi
    if k == 10:                                             # a column past 2^32
        s, f, v = rows[0]
        s[2:7], f[2:7], v[2:7] = 1, 1 + 2 ** 30, v[2]
    if k % 5 == 4:
        for r in rows:
            r[2][2:][rng.random(len(r[2]) - 2) < 0.3] = np.nan
        if k == 4:                                          # a NaN run leading row 0
            rows[0] = [np.concatenate([[5], rows[0][0]]).astype(np.int32), np.concatenate([[9], rows[0][1]]).astype(np.int32), np.concatenate([[np.nan], rows[0][2]])]
    if n_rows > 1 and k % 6 == 5:
        rows[-1] = [np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0)]
    if n_rows > 1 and k % 6 == 2:
        rows[-1][2][:] = np.nan
    return M.Lists.from_rows(rows), w


def main():
    ref = sys.argv[1]
    rng = np.random.default_rng(20261103)
    num = lambda x: None if x != x else float(x)      # noqa: E731
    out = {"generator": "tests/golden/make_hist_golden.py",
           "source": "compiled reference v1.2.11: histogram, print_histogram, normalize_histogram + print_histogram over array-backed children",
           "cases": []}
    seen = {"high_low": 0, "nan": 0, "equal": 0, "big": 0, "empty_row": 0, "nan_row": 0}
    with tempfile.TemporaryDirectory() as tmp:
        L = build(ref, tmp)
        for k in range(63):
            lists, w = make_case(rng, k)
            assert M.reference_equal(lists, w), k
            hist, r2, text, ntext = run(L, lists, w)
            (lo, hi), model = M.histogram(lists, w)
            assert M.same_bits(hist, model) and M.same_bits(r2, [lo, hi]), (k, hist, model, r2, lo, hi)
            assert text == M.text((lo, hi), model) and ntext == M.text((lo, hi), M.normalize(model)), k
            rows = lists.rows()
            ok = rows[0][2][~np.isnan(rows[0][2])]
            seen["high_low"] += int(len(ok) > 1 and ok[0] > ok[1])
            seen["nan"] += int(np.isnan(lists.v).any())
            seen["equal"] += int(lo == hi)
            seen["big"] += int(model.max() > 2.0 ** 32)
            seen["empty_row"] += int(any(len(r[0]) == 0 for r in rows))
            seen["nan_row"] += int(any(len(r[0]) and np.isnan(r[2]).all() for r in rows))
            out["cases"].append({"name": "case%03d" % k, "width": w,
                                 "rows": [{"start": r[0].tolist(), "finish": r[1].tolist(), "value": [num(x) for x in r[2].tolist()]} for r in rows],
                                 "range": [num(r2[0]), num(r2[1])], "hist": [[int(x) for x in row] for row in hist.tolist()],
                                 "text": text, "normalized_text": ntext})
    assert min(seen.values()) >= 1, seen
    path = os.path.join(HERE, "hist_fixtures.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    size = os.path.getsize(path)
    print("wrote %d cases, every matrix and range equal to the model bit for bit, %r, %d bytes" % (len(out["cases"]), seen, size))
    assert size < 250000, size
    for c in M.fixtures():                                  # what is stored reads back as what was recorded
        lists, w = M.fixture_lists(c)
        (lo, hi), model = M.histogram(lists, w)
        assert M.same_bits(M.fixture_result(c)[1], model) and M.same_bits(M.fixture_result(c)[0], [lo, hi]), c["name"]


if __name__ == "__main__":
    main()
