#!/usr/bin/env python
"""Generates tests/golden/profile_fixtures.json: small datasets and regions and the VERBATIM rows of the compiled reference's
ProfileMultiplexer (src/apply.c over regionProfile of src/plots.c; `profiles`) over them, with their running sum in the order
served (`profile`).

The driver is our own: the array-backed child iterators of make_apply_golden.py and a loop that pops the reference's
Multiplexer to its end.  It is compiled together with the reference's sources, unmodified and from where they lie, into a
shared object in a temporary directory.  Nothing compiled is kept.

Cases: the generators of the apply goldens (1-3 chromosomes, a chromosome missing on either side; overlapping, nested and
identical regions, tests/golden/overlapping.bed among them; regions in gaps, before the first run and after the last; edges on
run edges), values k / 8, NaN runs in every fifth case, every region shorter than 10^6 bp, defaults cycling 0, NaN, 1.5,
widths cycling 1, 2, 3, 7, 10, 64, 100, and in every case regions of length W / 2, W, 3 W / 2 + 1, 2 W and 5 W + 3 so that every
regime occurs: L < W, L == W, W < L < 2 W, L == 2 W, L > 2 W.  Rows are stored run-length encoded (rle()).

Prints the share of recorded bins that are not `exact` (profile_model.Bin.exact); it must be at most 40 %.

Run where the reference's sources are present:  python tests/golden/make_profile_golden.py <path to the reference>
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
import profile_model as PM  # noqa: E402
import region_model as RM  # noqa: E402
from make_coverage_golden import REF_SRCS, read_bed  # noqa: E402

WIDTHS = (1, 2, 3, 7, 10, 64, 100)
DEFAULTS = (0.0, float("nan"), 1.5)

DRIVER = AG.DRIVER + r'''
/* Returns the number of regions the Multiplexer served; o_values: width per region; o_sum: the rows added in the order served. */
long long golden_profile(int n_chrom, char **names, long long *seg_off, int *start, int *finish, double *value, double default_value,
                         int r_chrom, char **r_names, long long *r_seg_off, int *r_start, int *r_finish, double *r_value,
                         int width, long long cap, char **all_names, int n_all,
                         int *o_chrom, int *o_start, int *o_finish, double *o_values, double *o_sum) {
    WiggleIterator *data = arr_new(n_chrom, names, seg_off, start, finish, value, default_value);
    WiggleIterator *regions = arr_new(r_chrom, r_names, r_seg_off, r_start, r_finish, r_value, 0);
    Multiplexer *m = ProfileMultiplexer(regions, width, data);
    long long n = 0;
    for (int i = 0; i < width; i++) o_sum[i] = 0;
    while (!m->done) {
        if (n < cap) {
            int c = 0;
            while (c < n_all && strcmp(all_names[c], m->chrom)) c++;
            o_chrom[n] = c; o_start[n] = m->start; o_finish[n] = m->finish;
            for (int i = 0; i < width; i++) { o_values[n * width + i] = m->values[i]; o_sum[i] += m->values[i]; }
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
    so = os.path.join(tmp, "libprofilegold.so")
    subprocess.check_call(["gcc", "-g", "-w", "-O3", "-std=gnu99", "-fPIC", "-shared", "-I" + os.path.join(ref, "src")] +
                          [os.path.join(ref, "src", s) for s in REF_SRCS + ["apply.c", "plots.c"]] + [drv, "-o", so, "-lm", "-lpthread"])
    return C.CDLL(so, mode=os.RTLD_LAZY)


def run(L, all_names, data, regions, default, width):
    a, r = AG._side(*data), AG._side(regions[0], regions[1], np.ones(sum(len(p[0]) for p in regions[1])))
    cap = len(r[2]) + 8
    alln = (C.c_char_p * len(all_names))(*[x.encode() for x in all_names])
    oc, os_, of = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    ov, osum = np.zeros((cap, width), np.float64), np.zeros(width, np.float64)
    p = lambda x: C.c_void_p(x.ctypes.data)      # noqa: E731
    L.golden_profile.restype = C.c_longlong
    n = L.golden_profile(C.c_int(len(data[0])), a[0], p(a[1]), p(a[2]), p(a[3]), p(a[4]), C.c_double(default),
                         C.c_int(len(regions[0])), r[0], p(r[1]), p(r[2]), p(r[3]), p(r[4]),
                         C.c_int(width), C.c_longlong(cap), alln, C.c_int(len(all_names)), p(oc), p(os_), p(of), p(ov), p(osum))
    assert n == len(r[2]), (n, len(r[2]))
    num = lambda x: None if x != x else x      # noqa: E731
    return {"chrom": oc[:n].tolist(), "start": os_[:n].tolist(), "finish": of[:n].tolist(),
            "rows": [[num(x) for x in row] for row in ov[:n].tolist()], "sum": [num(x) for x in osum.tolist()]}


def rle(row):
    """A row for the file: a value, or [value, count] for count >= 2 consecutive bins with the same bits (a stretched position,
    a gap over several bins, empty bins)."""
    out, i = [], 0
    while i < len(row):
        j = i
        while j < len(row) and (row[j] is row[i] if row[i] is None or row[j] is None else np.float64(row[j]).tobytes() == np.float64(row[i]).tobytes()):
            j += 1
        out.append(row[i] if j - i == 1 else [row[i], j - i])
        i = j
    return out


def with_regimes(rng, regs, W, span):
    """The regions of a chromosome plus one of every regime of L against W."""
    rs, rf = (x.astype(np.int64) for x in regs)
    lens = [max(W // 2, 1), W, W + W // 2 + 1, 2 * W, 5 * W + 3]
    at = rng.integers(0, max(span - 1, 1), len(lens))
    rs, rf = np.concatenate([rs, at]), np.concatenate([rf, at + lens])
    o = np.argsort(rs, kind="stable")
    return rs[o].astype(np.int32), rf[o].astype(np.int32)


def main():
    ref = sys.argv[1]
    rng = np.random.default_rng(20261021)
    all_names = ["chr1", "chr2", "chr3"]
    cases = []
    bed_names, bed = read_bed(os.path.join(HERE, "overlapping.bed"))
    for k in range(120):
        span = int((30, 200, 3000)[k % 3])
        W = WIDTHS[k % len(WIDTHS)]
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
            regs = [AG.regions_for(rng, k, by_name.get(nm, empty), span, q == 0 or nm not in by_name) for q, nm in enumerate(names_r)]
            regs[0] = with_regimes(rng, regs[0], W, span)
            local_all = all_names
        n_d = sum(len(p[0]) for p in data)
        value = rng.integers(-80, 80, n_d) / 8.0                # exact in float32
        with_nan = k % 5 == 4
        if with_nan:
            value[rng.random(n_d) < 0.3] = np.nan
        default = DEFAULTS[(k // 2) % 3]
        cases.append(("case%03d" % k, local_all, (names_d, data, value), (names_r, regs), default, with_nan, W))
    out = {"generator": "tests/golden/make_profile_golden.py",
           "source": "compiled reference v1.2.11: ProfileMultiplexer over array-backed children, `width` values per region and their running sum",
           "cases": []}
    inexact = total = 0
    regimes = set()
    with tempfile.TemporaryDirectory() as tmp:
        L = build(ref, tmp)
        for name, local_all, data, regs, default, with_nan, W in cases:
            rec = {"name": name, "chrom_names": local_all, "default": None if default != default else default, "nan_values": with_nan, "width": W}
            d, r = AG._side(*data), AG._side(regs[0], regs[1], np.zeros(0))
            rec["data"] = {"chroms": [local_all.index(x) for x in data[0]], "seg_off": d[1].tolist(), "start": d[2].tolist(), "finish": d[3].tolist(),
                           "value": [None if x != x else x for x in d[4].tolist()]}
            rec["regions"] = {"chroms": [local_all.index(x) for x in regs[0]], "seg_off": r[1].tolist(), "start": r[2].tolist(), "finish": r[3].tolist()}
            rec.update(run(L, local_all, data, regs, default, W))
            case, dflt, _ = PM.fixture_case(rec)
            rec["rows"] = [rle(row) for row in rec["rows"]]
            out["cases"].append(rec)
            a, b = PM.Expected(case).inexact_share(W, dflt)
            inexact, total = inexact + a, total + b
            for x in (case.rf.astype(np.int64) - case.rs):
                regimes.add("L<W" if x < W else "L==W" if x == W else "W<L<2W" if x < 2 * W else "L==2W" if x == 2 * W else "L>2W")
    assert regimes == {"L<W", "L==W", "W<L<2W", "L==2W", "L>2W"}, regimes
    share = inexact / total
    print("%d of %d recorded bins are not exact: %.1f %%" % (inexact, total, 100 * share))
    assert share <= 0.40
    path = os.path.join(HERE, "profile_fixtures.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    print("wrote %d cases, %d bytes" % (len(out["cases"]), os.path.getsize(path)))


if __name__ == "__main__":
    main()
