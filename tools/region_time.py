"""Times the region door (csrc/wt_region.hip, wtamd_runs_region) on the GPU, wtamd_runs_map with WTAMD_MAP_GT over the same
list in the same process (the same ordered compaction without a search), and the compiled reference's Overlap / Noverlap /
Trim / NearestWiggleIterator over the same input on the same host where oracle/_ref holds it.

Input (one segment): a source of 6 * 10^7 runs that do not overlap (f32 values), resident in HBM, against masks of 10^3, 10^5
and 10^7 intervals that cover some 30 % of the span.  Every door is timed with events around the whole call (its device
allocations, the union of the mask, its passes and the copies of its counters included), --reps times after one warm-up; the
minimum counts.  GB/s = (12 bytes per source run read + 16 bytes per run written) / time.  The reference is driven by a small
C driver of our own (array-backed children, the iterator popped to its end), built into a temporary directory against
include/wiggletools_amd.h, whose struct layout is the reference's; one thread.

  python tools/region_time.py [--out profiles/region.json] [--reps 3] [--runs 60000000] [--no-reference]
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

OPS = ("overlaps", "noverlaps", "trim", "nearest")
MAP_GT = 8

DRIVER = r'''
#include <stdlib.h>
#include "wiggletools_amd.h"
extern WiggleIterator *OverlapWiggleIterator(WiggleIterator *, WiggleIterator *);
extern WiggleIterator *NoverlapWiggleIterator(WiggleIterator *, WiggleIterator *);
extern WiggleIterator *TrimWiggleIterator(WiggleIterator *, WiggleIterator *);
extern WiggleIterator *NearestWiggleIterator(WiggleIterator *, WiggleIterator *);
typedef struct { long long n, j; const int *start, *finish; const float *value; char *chrom; } Arr;
static void arr_pop(WiggleIterator *wi) {
    Arr *a = (Arr *) wi->data;
    if (a->j >= a->n) { wi->done = 1; return; }
    wi->chrom = a->chrom; wi->start = a->start[a->j]; wi->finish = a->finish[a->j]; wi->value = a->value ? a->value[a->j] : 1; a->j++;
}
static void arr_seek(WiggleIterator *wi, const char *c, int s, int f) { }
static WiggleIterator *arr_new(long long n, const int *start, const int *finish, const float *value, int overlaps) {
    Arr *a = (Arr *) calloc(1, sizeof(Arr));
    a->n = n; a->start = start; a->finish = finish; a->value = value; a->chrom = "chr1";
    return newWiggleIterator(a, &arr_pop, &arr_seek, 0, overlaps);
}
long long ref_region(int op, long long n, const int *start, const int *finish, const float *value, long long m, const int *m_start,
                     const int *m_finish, double *bp) {
    WiggleIterator *src = arr_new(n, start, finish, value, 0), *mask = arr_new(m, m_start, m_finish, 0, 1);
    WiggleIterator *wi = op == 0 ? OverlapWiggleIterator(src, mask) : op == 1 ? NoverlapWiggleIterator(src, mask)
                       : op == 2 ? TrimWiggleIterator(src, mask) : NearestWiggleIterator(src, mask);
    long long runs = 0;
    double acc = 0;
    while (!wi->done) { runs++; acc += (double) (wi->finish - wi->start); pop(wi); }
    *bp = acc;
    return runs;
}
'''


def make_source(rng, n):
    gap, ln = rng.integers(0, 30, n), rng.integers(1, 30, n)          # 0: the run touches the one before it
    s = 1 + np.cumsum(gap + ln) - ln
    assert s[-1] + ln[-1] < 2 ** 31
    return s.astype(np.int32), (s + ln).astype(np.int32), rng.standard_normal(n).astype(np.float32)


def make_mask(rng, m, span):
    s = np.sort(rng.integers(1, span, m))
    ln = np.maximum(rng.poisson(0.3 * span / m, m), 1)
    return s.astype(np.int32), np.minimum(s + ln, 2 ** 31 - 1).astype(np.int32)


def timed(reps, call):
    import torch
    ms = []
    for k in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        if k:
            ms.append(e0.elapsed_time(e1))
    return ms


def time_reference(op, s, f, v, ms, mf):
    ref = os.path.join(ROOT, "oracle", "_ref", "libwiggletools_ref.so")
    if not os.path.exists(ref):
        return None
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "d.c"), "w").write(DRIVER)
        so = os.path.join(tmp, "libregtime.so")
        subprocess.check_call(["gcc", "-O2", "-w", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), os.path.join(tmp, "d.c"), "-o", so])
        C.CDLL(ref, mode=os.RTLD_LAZY | os.RTLD_GLOBAL)
        D = C.CDLL(so, mode=os.RTLD_LAZY | os.RTLD_GLOBAL)
        D.ref_region.restype = C.c_longlong
        p = lambda a: C.c_void_p(a.ctypes.data)      # noqa: E731
        acc = C.c_double()
        t0 = time.perf_counter()
        runs = D.ref_region(C.c_int(op), C.c_longlong(len(s)), p(s), p(f), p(v), C.c_longlong(len(ms)), p(ms), p(mf), C.byref(acc))
        dt = time.perf_counter() - t0
    return {"runs": runs, "bp": acc.value, "seconds": dt, "source_runs_per_s": len(s) / dt}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--runs", type=int, default=60_000_000)
    ap.add_argument("--no-reference", action="store_true")
    a = ap.parse_args()
    import torch
    from wiggletools_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2026)
    s, f, v = make_source(rng, a.runs)
    n, span = len(s), int(f[-1])
    ds, df, dv = torch.from_numpy(s).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(v).to(dev)
    seg, oseg, n_out = np.array([0, n], np.int64), np.zeros(2, np.int64), C.c_int64()
    cap = n + 10_000_000
    os_ = torch.empty(cap, dtype=torch.int32, device=dev)
    of = torch.empty(cap, dtype=torch.int32, device=dev)
    ov = torch.empty(cap, dtype=torch.float64, device=dev)
    rec = {"tool": "tools/region_time.py", "device": torch.cuda.get_device_name(0), "source_runs": n, "span_bp": span, "value": "f32",
           "timing": "events around the call, allocations included; minimum of --reps after one warm-up",
           "GB_per_s": "(12 B per source run read + 16 B per run written) / time"}
    # the yardstick: the same ordered compaction without a search
    ms_map = timed(a.reps, lambda: _lib.check(L.wtamd_runs_map(MAP_GT, 0.0, 1, seg.ctypes.data, ds.data_ptr(), df.data_ptr(), dv.data_ptr(), 0,
                                                               os_.data_ptr(), of.data_ptr(), ov.data_ptr(), oseg.ctypes.data, None)))
    best = min(ms_map) * 1e-3
    rec["map_gt"] = {"ms": ms_map, "best_ms": min(ms_map), "runs_out": int(oseg[1]), "GB_per_s": (12.0 * n + 16.0 * int(oseg[1])) / best / 1e9}
    print(json.dumps({"map_gt": rec["map_gt"]}), flush=True)
    for m in (1_000, 100_000, 10_000_000):
        ms_, mf_ = make_mask(rng, m, span)
        dms, dmf = torch.from_numpy(ms_).to(dev), torch.from_numpy(mf_).to(dev)
        mseg = np.array([0, m], np.int64)
        per = {}
        for op, name in enumerate(OPS):
            t = timed(a.reps, lambda: _lib.check(L.wtamd_runs_region(op, 1, seg.ctypes.data, ds.data_ptr(), df.data_ptr(), dv.data_ptr(), 0,
                                                                     mseg.ctypes.data, dms.data_ptr(), dmf.data_ptr(), cap, os_.data_ptr(),
                                                                     of.data_ptr(), ov.data_ptr(), oseg.ctypes.data, C.byref(n_out), None)))
            k = n_out.value
            best = min(t) * 1e-3
            r = {"ms": t, "best_ms": min(t), "runs_out": k, "bp_out": float((of[:k] - os_[:k]).double().sum().item()),
                 "source_runs_per_s": n / best, "GB_per_s": (12.0 * n + 16.0 * k) / best / 1e9, "time_over_map_gt": min(t) / min(ms_map)}
            if not a.no_reference:
                ref = time_reference(op, s, f, v, ms_, mf_)
                if ref:
                    assert ref["runs"] == k and ref["bp"] == r["bp_out"], (name, ref, r)      # the same list
                    r["reference_1_thread"] = ref
                    r["device_over_reference"] = r["source_runs_per_s"] / ref["source_runs_per_s"]
            per[name] = r
            print(json.dumps({"mask_%d" % m: {name: r}}), flush=True)
        rec["mask_%d" % m] = per
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
