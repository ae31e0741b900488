"""Times the window doors (csrc/wt_window.hip: wtamd_runs_bin, wtamd_runs_smooth) on the GPU.

bin: the dataset tools/region_time.py builds -- 6 * 10^7 runs that do not overlap, f32 values, resident in HBM, one segment -- at
widths 10, 10^3 and 10^6, as runs per second and as the ratio to wtamd_runs_map GT over the same list in the same process: the
same read and an ordered compaction, without a window.
smooth: widths 10 and 1000 over the prefix of that dataset that spans 2.5 * 10^8 bp (one chromosome; 4 GB of output), as GB/s
counting 12 bytes per run read plus 16 bytes per position written.
Every call is timed with events around the whole call (its pool allocations, its passes and the copies of its counters
included), --reps times after one warm-up; the minimum counts.

With --reference <the reference's sources> the compiled reference's BinningWiggleIterator / SmoothWiggleIterator are timed INSTEAD,
on this host's CPU, on one thread, through the driver of tests/golden/make_window_golden.py (array children, the pops counted and
nothing stored), over the same runs -- or, with --ref-runs N, over a PREFIX of N runs: the ratios to the device are then
EXTRAPOLATED from that prefix and labelled so.  It needs no GPU and adds its figures to the file the device run wrote.

  python tools/window_time.py [--out profiles/window.json] [--reps 3] [--runs 60000000] [--reference PATH]
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from region_time import make_source, timed  # noqa: E402

BIN_WIDTHS = (10, 1000, 1000000)
SMOOTH_WIDTHS = (10, 1000)
SMOOTH_BP = 250_000_000


def reference(a, s, f, v):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import make_window_golden as G
    import window_model as M
    out = {}
    kb = min(a.ref_runs, len(s)) if a.ref_runs else len(s)
    ks = min(kb, int(np.searchsorted(f.astype(np.int64), SMOOTH_BP)))
    cases = {0: M.Case([(s[:kb], f[:kb], v[:kb].astype(np.float64))]), 1: M.Case([(s[:ks], f[:ks], v[:ks].astype(np.float64))])}
    p = lambda x: C.c_void_p(x.ctypes.data)      # noqa: E731
    arr = (C.c_char_p * 1)(b"chr1")
    with tempfile.TemporaryDirectory() as tmp:
        L = G.build(a.reference, tmp)
        L.golden_window.restype = C.c_longlong
        for op, widths in ((0, BIN_WIDTHS), (1, SMOOTH_WIDTHS)):
            case, k = cases[op], (ks if op else kb)
            for w in widths:
                t0 = time.perf_counter()              # (capacity 0: the pops are counted, nothing is stored)
                rows = L.golden_window(C.c_int(op), C.c_int(1), arr, p(case.seg), p(case.s), p(case.f), p(case.v), C.c_double(0.0), C.c_int(w),
                                       C.c_int(-1), C.c_int(0), C.c_int(0), C.c_longlong(0), None, None, None, None)
                dt = time.perf_counter() - t0
                name = "%s_w%d" % ("smooth" if op else "bin", w)
                out[name] = {"runs": k, "span_bp": int(f[k - 1]), "outputs": rows, "seconds": dt, "runs_per_s": k / dt, "outputs_per_s": rows / dt}
                print(json.dumps({"reference": {name: out[name]}}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--runs", type=int, default=60_000_000)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--ref-runs", type=int, default=0)
    a = ap.parse_args()
    rng = np.random.default_rng(2026)
    s, f, v = make_source(rng, a.runs)
    n = len(s)
    if a.reference:
        rec = json.load(open(a.out)) if os.path.exists(a.out) else {"tool": "tools/window_time.py"}
        rec["reference_1_thread"] = {"what": "the compiled reference's iterators over array children, popped to the end, nothing stored; on the CPU of the "
                                             "host that ran --reference (not the GPU host); " +
                                             ("a PREFIX of %d runs: the device_over_reference figures are ratios of rates EXTRAPOLATED from that prefix, "
                                              "not of like-for-like times" % a.ref_runs if a.ref_runs else "the same runs as the device"),
                                     "shapes": reference(a, s, f, v)}
        for name, d in rec["reference_1_thread"]["shapes"].items():
            if name in rec:
                key = "runs_per_s" if name.startswith("bin") else "outputs_per_s"
                rec[name]["device_over_reference_" + key] = rec[name][key] / d[key]
        json.dump(rec, open(a.out, "w"), indent=1)
        return
    import torch
    from wiggletools_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    ds, df, dv = torch.from_numpy(s).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(v).to(dev)
    seg, oseg, n_out = np.array([0, n], np.int64), np.zeros(2, np.int64), C.c_int64()
    rec = {"tool": "tools/window_time.py", "device": torch.cuda.get_device_name(0), "dataset_runs": n, "span_bp": int(f[-1]), "value": "f32",
           "timing": "events around the call, pool allocations included; minimum of --reps after one warm-up"}
    os_, of, ov = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    t = timed(a.reps, lambda: _lib.check(L.wtamd_runs_map(8, 0.0, 1, seg.ctypes.data, ds.data_ptr(), df.data_ptr(), dv.data_ptr(), 0, os_.data_ptr(),
                                                          of.data_ptr(), ov.data_ptr(), oseg.ctypes.data, None)))
    rec["map_gt"] = {"ms": t, "best_ms": min(t), "runs_per_s": n / (min(t) * 1e-3), "runs_out": int(oseg[1])}
    print(json.dumps({"map_gt": rec["map_gt"]}), flush=True)
    del os_, of, ov
    s64, f64 = s.astype(np.int64), f.astype(np.int64)
    for w in BIN_WIDTHS:
        cap = int(((f64 - 2) // w - (s64 - 1) // w + 1).sum())
        os_, of, ov = torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.float64, device=dev)
        t = timed(a.reps, lambda: _lib.check(L.wtamd_runs_bin(1, seg.ctypes.data, ds.data_ptr(), df.data_ptr(), dv.data_ptr(), 0, w, 0.0, cap, os_.data_ptr(),
                                                              of.data_ptr(), ov.data_ptr(), oseg.ctypes.data, C.byref(n_out), None)))
        best = min(t) * 1e-3
        rec["bin_w%d" % w] = {"width": w, "ms": t, "best_ms": min(t), "runs_per_s": n / best, "bins_out": n_out.value, "capacity": cap,
                              "GB_per_s": (12.0 * n + 16.0 * n_out.value) / best / 1e9, "time_over_map_gt": min(t) / rec["map_gt"]["best_ms"],
                              "first_values": ov[:4].cpu().tolist()}
        print(json.dumps({"bin_w%d" % w: rec["bin_w%d" % w]}), flush=True)
        del os_, of, ov
    k = int(np.searchsorted(f64, SMOOTH_BP))
    sseg = np.array([0, k], np.int64)
    for w in SMOOTH_WIDTHS:
        cap = int(f64[k - 1]) - max(1, int(s64[0]) - w // 2) + w
        os_, of, ov = torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.float64, device=dev)
        t = timed(a.reps, lambda: _lib.check(L.wtamd_runs_smooth(1, sseg.ctypes.data, ds.data_ptr(), df.data_ptr(), dv.data_ptr(), 0, w, 0, 0, cap, os_.data_ptr(),
                                                                 of.data_ptr(), ov.data_ptr(), oseg.ctypes.data, C.byref(n_out), None)))
        best = min(t) * 1e-3
        rec["smooth_w%d" % w] = {"width": w, "runs": k, "span_bp": int(f64[k - 1]), "ms": t, "best_ms": min(t), "outputs": n_out.value,
                                 "outputs_per_s": n_out.value / best, "bytes_written": 16 * n_out.value,
                                 "GB_per_s": (12.0 * k + 16.0 * n_out.value) / best / 1e9, "first_values": ov[:4].cpu().tolist()}
        print(json.dumps({"smooth_w%d" % w: rec["smooth_w%d" % w]}), flush=True)
        del os_, of, ov
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
