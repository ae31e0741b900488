"""Times the text door (csrc/wt_text.hip: wtamd_runs_text) on the GPU.

The dataset tools/region_time.py builds -- 6 * 10^7 runs, f32 values, resident in HBM, one segment -- in bedGraph mode, and in
wig mode over a second list of the same size with a realistic share of short runs (40 % of the runs are 1 to 3 bp long, so the
writer changes mode all the time and about a quarter of the entries are printed point by point).  Reported per shape: the bytes
written, runs per second, and GB/s counting the 12 bytes read per run plus the bytes written.  Every call is timed with events
around the whole call (its pool allocations, its three passes, the copies of its tables and scalars included), --reps times
after one warm-up per shape: minimum, median and (max - min) / min are kept.  A call with no room (capacity 0) runs the measure
and scan passes only and is timed the same way: the emit pass by difference.  The kernels' own durations come from a kernel
trace, a run of this tool per shape under `rocprofv3 --kernel-trace --stats` (--shape), whose kernel_stats.csv --kernel-trace
adds to the file.  Beside it,
wtamd_runs_map GT over the same list in the same process: the same read and an ordered compaction, without formatting.  The
text of a prefix of --check-runs runs is compared byte for byte with tests/text_model.py.

With --reference <the reference's sources> the compiled reference's TeeWiggleIterator is timed INSTEAD, on this host's CPU,
through the driver of tests/golden/make_text_golden.py (an array child) into /dev/null, over the same runs -- or, with
--ref-runs N, over a PREFIX of N runs: the ratios to the device are then ratios of RATES, EXTRAPOLATED from that prefix and
labelled so.  It needs no GPU and adds its figures to the file the device run wrote.

  python tools/text_time.py [--out profiles/text.json] [--reps 5] [--runs 60000000] [--reference PATH] [--ref-runs N]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from region_time import make_source, timed  # noqa: E402

DEVNULL_DRIVER = r'''
/* Returns the number of runs passed on. */
long long time_text(int n_chrom, char **names, long long *seg_off, int *start, int *finish, double *value, int bedGraph) {
    FILE *fp = fopen("/dev/null", "w");
    WiggleIterator *wi = TeeWiggleIterator(arr_new(n_chrom, names, seg_off, start, finish, value, 0), fp, bedGraph, false);
    long long n = 0;
    while (!wi->done) { n++; pop(wi); }
    fclose(fp);
    return n;
}
'''


def make_short(rng, n):
    """The wig list: 40 % of the runs 1 .. 3 bp, the others 1 .. 29; a third of them touch the run before."""
    ln = np.where(rng.random(n) < 0.4, rng.integers(1, 4, n), rng.integers(1, 30, n))
    gap = np.where(rng.random(n) < 0.33, 0, rng.integers(1, 12, n))
    s = 1 + np.cumsum(gap + ln) - ln
    assert s[-1] + ln[-1] < 2 ** 31
    return s.astype(np.int32), (s + ln).astype(np.int32), (rng.integers(0, 4000, n) / 16.0).astype(np.float32)


def reference(a, shapes):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_text_golden as G
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        drv = os.path.join(tmp, "driver.c")
        open(drv, "w").write(G.DRIVER + DEVNULL_DRIVER)
        so = os.path.join(tmp, "libtexttime.so")
        subprocess.check_call(["gcc", "-g", "-w", "-O3", "-std=gnu99", "-D_GNU_SOURCE", "-fPIC", "-shared", "-I" + os.path.join(a.reference, "src")] +
                              [os.path.join(a.reference, "src", x) for x in G.REF_SRCS] + [drv, "-o", so, "-lm", "-lpthread"])
        L = C.CDLL(so, mode=os.RTLD_LAZY)
        L.time_text.restype = C.c_longlong
        for name, (s, f, v, bed) in shapes.items():
            k = min(a.ref_runs, len(s)) if a.ref_runs else len(s)
            names = (C.c_char_p * 1)(b"chr1")
            seg = np.array([0, k], np.int64)
            v64 = v[:k].astype(np.float64)
            p = lambda x: C.c_void_p(x.ctypes.data)      # noqa: E731
            t0 = time.perf_counter()
            n = L.time_text(1, names, p(seg), p(s), p(f), p(v64), int(bed))
            dt = time.perf_counter() - t0
            out[name] = {"runs": k, "runs_passed_on": int(n), "seconds": dt, "runs_per_s": k / dt}
            print(json.dumps({"reference": {name: out[name]}}), flush=True)
    return out


def add_kernel_trace(a):
    """The kernels' own durations from `rocprofv3 --kernel-trace --stats -- python tools/text_time.py --shape SHAPE`, one run
    per shape: wt_text_kernel<0> is measure, <1> scan, <2> emit."""
    import csv
    rec = json.load(open(a.out))
    names = {"0": "measure", "1": "scan", "2": "emit"}
    out = {"what": "rocprofv3 --kernel-trace --stats, one run of this tool per shape in a process of its own (--shape), the warm-up calls and the calls "
                   "with no room included: a kernel's duration in microseconds, mean / min / max over its launches"}
    for item in a.kernel_trace.split(","):
        shape, path = item.split("=")
        d = {}
        for row in csv.DictReader(open(path)):
            for k, what in names.items():
                if "wt_text_kernel<%s>" % k in row["Name"] or "wt_text_kernelILi%sE" % k in row["Name"]:
                    d[what] = {"launches": int(row["Calls"]), "mean_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                               "max_us": float(row["MaxNs"]) / 1e3}
        assert len(d) == 3, (shape, d)
        out[shape] = d
    rec["kernel_trace"] = out
    json.dump(rec, open(a.out, "w"), indent=1)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=60_000_000)
    ap.add_argument("--check-runs", type=int, default=200_000)
    ap.add_argument("--shape", default=None, help="time this shape only (a run under a kernel trace)")
    ap.add_argument("--kernel-trace", default=None, help="SHAPE=kernel_stats.csv[,...]: adds the trace's kernel durations to --out and returns")
    ap.add_argument("--reference", default=None)
    ap.add_argument("--ref-runs", type=int, default=0)
    a = ap.parse_args()
    if a.kernel_trace:
        add_kernel_trace(a)
        return
    rng = np.random.default_rng(2026)
    s, f, v = make_source(rng, a.runs)
    ws, wf, wv = make_short(rng, a.runs)
    n = len(s)
    shapes = {"bedgraph": (s, f, v, True), "wig_short_runs": (ws, wf, wv, False)}
    if a.shape:
        shapes = {a.shape: shapes[a.shape]}
    if a.reference:
        rec = json.load(open(a.out)) if os.path.exists(a.out) else {"tool": "tools/text_time.py"}
        ref = reference(a, shapes)
        rec["reference_1_thread"] = {"what": "the compiled reference's TeeWiggleIterator (its compression rule in front in wig mode, its writer thread printing) "
                                             "over an array child into /dev/null, popped to the end; on the CPU of the host that ran --reference (not the GPU "
                                             "host); " + ("EXTRAPOLATED: a PREFIX of %d runs, the device_over_reference figures are ratios of RATES, not of "
                                                          "like-for-like times" % a.ref_runs if a.ref_runs else "the same runs as the device"),
                                     "shapes": ref}
        for name, d in ref.items():
            if name in rec.get("shapes", {}):
                rec["shapes"][name]["device_over_reference_runs_per_s"] = rec["shapes"][name]["runs_per_s"] / d["runs_per_s"]
        json.dump(rec, open(a.out, "w"), indent=1)
        return
    import torch
    import text_model as M
    from wiggletools_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    rec = {"tool": "tools/text_time.py", "device": torch.cuda.get_device_name(0), "dataset_runs": n, "value": "f32", "reps": a.reps,
           "timing": "events around the call, pool allocations included; --reps after one warm-up per shape: ms lists every repeat, best_ms the minimum, "
                     "spread = (max - min) / min; measure_and_scan: the same call with capacity 0, which stops after the scan; emit_by_difference: the difference "
                     "of the two minima; kernel_trace (added by --kernel-trace): the kernels' own durations",
           "GB_per_s": "(12 B per run + the bytes written) / time", "shapes": {}}
    names = (C.c_char_p * 1)(b"chr1")
    seg = np.array([0, n], np.int64)
    for name, (hs, hf, hv, bed) in shapes.items():
        ds, df, dv = torch.from_numpy(hs).to(dev), torch.from_numpy(hf).to(dev), torch.from_numpy(hv).to(dev)
        flags = 1 if bed else 0
        nb, nw = C.c_int64(), C.c_int64()

        def call(text, cap, want):
            rc = L.wtamd_runs_text(1, seg.ctypes.data, names, ds.data_ptr(), df.data_ptr(), dv.data_ptr(), 0, flags, None, text, cap, C.byref(nb), C.byref(nw), None)
            assert rc == want, (rc, L.wtamd_last_error())

        t_ms = timed(a.reps, lambda: call(None, 0, 3))
        size = int(nb.value)
        text = torch.empty(size, dtype=torch.uint8, device=dev)
        t = timed(a.reps, lambda: call(text.data_ptr(), size, 0))
        best = min(t) * 1e-3
        d = {"mode": "bedGraph" if bed else "wig", "bytes": size, "bytes_per_run": size / n, "ms": t, "best_ms": min(t), "median_ms": float(np.median(t)),
             "spread": (max(t) - min(t)) / min(t), "runs_per_s": n / best, "GB_per_s": (12.0 * n + size) / best / 1e9,
             "measure_and_scan": {"ms": t_ms, "best_ms": min(t_ms)}, "emit_by_difference_ms": min(t) - min(t_ms)}
        # the same read and an ordered compaction, without formatting
        os_, of = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        ov, oseg = torch.empty(n, dtype=torch.float64, device=dev), np.zeros(2, np.int64)
        tm = timed(a.reps, lambda: _lib.check(L.wtamd_runs_map(8, 0.0, 1, seg.ctypes.data, ds.data_ptr(), df.data_ptr(), dv.data_ptr(), 0, os_.data_ptr(),
                                                               of.data_ptr(), ov.data_ptr(), oseg.ctypes.data, None)))
        d["map_gt"] = {"ms": tm, "best_ms": min(tm), "runs_out": int(oseg[1])}
        d["time_over_map_gt"] = min(t) / min(tm)
        del os_, of, ov
        # a prefix against the model, byte for byte (a prefix of whole blocks prints what the whole list prints there)
        k = min(a.check_runs // M.BLOCK * M.BLOCK, n)
        if k:
            want = M.text(M.Lists(["chr1"], [0, k], hs[:k], hf[:k], hv[:k].astype(np.float64)), flags)[0]
            d["prefix_checked_runs"] = k
            d["prefix_equal_to_model_byte_for_byte"] = bool(text[:len(want)].cpu().numpy().tobytes() == want)
        rec["shapes"][name] = d
        print(json.dumps({name: d}), flush=True)
        del text, ds, df, dv
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
