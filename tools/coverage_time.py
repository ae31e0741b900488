"""Times the coverage door (csrc/wt_cover.hip, wtamd_runs_coverage) on the GPU, and the compiled reference's
CoverageWiggleIterator over the same input on the same host where oracle/_ref holds it.

Inputs (one segment each):
  reads    10^7 intervals, mean length 150, over 2.5 * 10^8 bp -- read-like
  sparse   10^4 intervals over the same span: the bitmap passes dominate
The door is timed with events around the whole call (its device allocations, its passes and the copies of its counters
included), --reps times after one warm-up; the minimum counts.  intervals/s; GB/s = (8 bytes per interval read + 16 bytes per
run written) / time.  The reference is driven by a small C driver of our own (an array-backed child with `overlaps` set,
the iterator popped to its end), built into a temporary directory against include/wiggletools_amd.h, whose struct layout is
the reference's.

  python tools/coverage_time.py [--out profiles/coverage.json] [--reps 5] [--no-reference]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DRIVER = r'''
#include <stdlib.h>
#include "wiggletools_amd.h"
extern WiggleIterator *CoverageWiggleIterator(WiggleIterator *);
typedef struct { long long n, j; const int *start, *finish; char *chrom; } Arr;
static void arr_pop(WiggleIterator *wi) {
    Arr *a = (Arr *) wi->data;
    if (a->j >= a->n) { wi->done = 1; return; }
    wi->chrom = a->chrom; wi->start = a->start[a->j]; wi->finish = a->finish[a->j]; wi->value = 1; a->j++;
}
static void arr_seek(WiggleIterator *wi, const char *c, int s, int f) { }
long long ref_coverage(long long n, const int *start, const int *finish, double *depth_bp) {
    Arr *a = (Arr *) calloc(1, sizeof(Arr));
    a->n = n; a->start = start; a->finish = finish; a->chrom = "chr1";
    WiggleIterator *wi = CoverageWiggleIterator(newWiggleIterator(a, &arr_pop, &arr_seek, 0, 1));
    long long runs = 0;
    double acc = 0;
    while (!wi->done) { runs++; acc += (double) (wi->finish - wi->start) * wi->value; pop(wi); }
    *depth_bp = acc;
    return runs;
}
'''


def make_input(rng, n, span, mean_len):
    s = np.sort(rng.integers(1, span, n)).astype(np.int32)
    f = (s + np.maximum(rng.poisson(mean_len, n), 1)).astype(np.int32)
    return s, f


def time_door(s, f, reps):
    import torch
    from wiggletools_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    n = len(s)
    ds, df = torch.from_numpy(s).to(dev), torch.from_numpy(f).to(dev)
    cap = 2 * n - 1
    os_ = torch.empty(cap, dtype=torch.int32, device=dev)
    of = torch.empty(cap, dtype=torch.int32, device=dev)
    ov = torch.empty(cap, dtype=torch.float64, device=dev)
    seg, oseg, n_out = np.array([0, n], np.int64), np.zeros(2, np.int64), C.c_int64()
    ms = []
    for k in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(L.wtamd_runs_coverage(1, seg.ctypes.data, ds.data_ptr(), df.data_ptr(), cap, os_.data_ptr(), of.data_ptr(), ov.data_ptr(),
                                         oseg.ctypes.data, C.byref(n_out), None))
        e1.record()
        e1.synchronize()
        if k:
            ms.append(e0.elapsed_time(e1))
    m = n_out.value
    depth_bp = float(((of[:m] - os_[:m]).double() * ov[:m]).sum().item())
    best = min(ms) * 1e-3
    return {"intervals": n, "runs": m, "depth_bp": depth_bp, "ms": ms, "best_ms": min(ms), "intervals_per_s": n / best,
            "GB_per_s": (8.0 * n + 16.0 * m) / best / 1e9}


def time_reference(s, f):
    ref = os.path.join(ROOT, "oracle", "_ref", "libwiggletools_ref.so")
    if not os.path.exists(ref):
        return None
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "d.c"), "w").write(DRIVER)
        so = os.path.join(tmp, "libcovtime.so")
        subprocess.check_call(["gcc", "-O2", "-w", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), os.path.join(tmp, "d.c"), "-o", so])
        C.CDLL(ref, mode=os.RTLD_LAZY | os.RTLD_GLOBAL)
        D = C.CDLL(so, mode=os.RTLD_LAZY | os.RTLD_GLOBAL)
        D.ref_coverage.restype = C.c_longlong
        acc = C.c_double()
        t0 = time.perf_counter()
        runs = D.ref_coverage(C.c_longlong(len(s)), C.c_void_p(s.ctypes.data), C.c_void_p(f.ctypes.data), C.byref(acc))
        dt = time.perf_counter() - t0
    return {"runs_with_its_zero_length_run": runs, "depth_bp": acc.value, "seconds": dt, "intervals_per_s": len(s) / dt}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coverage.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--span", type=int, default=250_000_000)
    ap.add_argument("--no-reference", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(2026)
    rec = {"tool": "tools/coverage_time.py", "span_bp": a.span, "timing": "events around wtamd_runs_coverage, allocations included; minimum of --reps"}
    for name, n in (("reads", 10_000_000), ("sparse", 10_000)):
        s, f = make_input(rng, n, a.span, 150)
        r = time_door(s, f, a.reps)
        if not a.no_reference:
            ref = time_reference(s, f)
            if ref:
                assert ref["depth_bp"] == r["depth_bp"], (ref, r)        # the same depth track (its zero-length run adds 0)
                r["reference"] = ref
                r["device_over_reference"] = r["intervals_per_s"] / ref["intervals_per_s"]
        rec[name] = r
        print(json.dumps({name: r}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
