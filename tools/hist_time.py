"""Times the histogram door (csrc/wt_hist.hip: wtamd_runs_histogram) on the GPU.

The dataset tools/region_time.py builds -- 6 * 10^7 runs, f32 values, resident in HBM -- as one row (one segment) and as 10 rows
(ten segments of equal size), at widths 10, 100, WHS_LDS_WIDTH and 10^6 (the global regime), with two value sets over the same
runs: `uniform` over [0, 1), and `skewed`, coverage-like, 90 % of the runs at 1.0 and the rest whole numbers 0 .. 50.  Reported
per shape: runs per second; GB/s counting the 12 bytes per run the two passes each READ ONCE (so the figure is what a single
read would need, not the traffic); the time as a multiple of wtamd_runs_moments over the same list in the same process (f64
values: 16 bytes per run streamed once, nothing scattered); per width and row count, skewed over uniform.  Every call is
timed with events around the whole call (its pool allocations, its passes, the copy of its scalars and the zeroing and
conversion of the matrix included), --reps times after one warm-up per shape: minimum, median and (max - min) / min are kept.
Every timed result is compared, bit for bit, with NumPy's histogram of the same columns (--no-check skips that).

With --reference <the reference's sources> the compiled reference's histogram() is timed INSTEAD, on this host's CPU, on one
thread, through the driver of tests/golden/make_hist_golden.py (array children), over the same runs -- or, with --ref-runs N,
over a PREFIX of N runs: the ratios to the device are then ratios of RATES, extrapolated from that prefix and labelled so.  It
needs no GPU and adds its figures to the file the device run wrote.

  python tools/hist_time.py [--out profiles/histogram.json] [--reps 5] [--runs 60000000] [--reference PATH] [--ref-runs N]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from region_time import make_source, timed  # noqa: E402

ROWS = (1, 10)


def value_sets(rng, n):
    uniform = rng.random(n, dtype=np.float32)
    skewed = np.where(rng.random(n) < 0.9, 1.0, rng.integers(0, 51, n)).astype(np.float32)
    return {"uniform": uniform, "skewed": skewed}


def reference(a, s, f, values, widths):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import hist_model as M
    import make_hist_golden as G
    k = min(a.ref_runs, len(s)) if a.ref_runs else len(s)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        L = G.build(a.reference, tmp)
        for kind, v in values.items():
            for rows in ROWS:
                seg = np.linspace(0, k, rows + 1).astype(np.int64)
                lists = M.Lists(seg, np.arange(rows), rows, s[:k], f[:k], v[:k].astype(np.float64))
                for w in widths:
                    t0 = time.perf_counter()
                    G.run(L, lists, w)
                    dt = time.perf_counter() - t0
                    name = "%s_rows%d_w%d" % (kind, rows, w)
                    out[name] = {"runs": k, "seconds": dt, "runs_per_s": k / dt}
                    print(json.dumps({"reference": {name: out[name]}}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "histogram.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=60_000_000)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--ref-runs", type=int, default=0)
    ap.add_argument("--ref-widths", default="10,100")
    ap.add_argument("--no-check", action="store_true")
    a = ap.parse_args()
    import hist_model as M
    lds_width = M.constants()["LDS_WIDTH"]
    widths = (10, 100, lds_width, 1000000)
    rng = np.random.default_rng(2026)
    s, f, _ = make_source(rng, a.runs)
    n = len(s)
    values = value_sets(rng, n)
    if a.reference:
        rec = json.load(open(a.out)) if os.path.exists(a.out) else {"tool": "tools/hist_time.py"}
        shapes = reference(a, s, f, values, [int(x) for x in a.ref_widths.split(",")])
        rec["reference_1_thread"] = {"what": "the compiled reference's histogram() over array children (print_histogram and normalize_histogram of the "
                                             "fixture driver included: microseconds); on the CPU of the host that ran --reference (not the GPU host), one "
                                             "thread; " + ("a PREFIX of %d runs: the device_over_reference figures are ratios of RATES extrapolated from "
                                                           "that prefix, not of like-for-like times" % a.ref_runs if a.ref_runs else "the same runs as the device"),
                                     "shapes": shapes}
        for name, d in shapes.items():
            if name in rec.get("shapes", {}):
                rec["shapes"][name]["device_over_reference_runs_per_s"] = rec["shapes"][name]["runs_per_s"] / d["runs_per_s"]
        json.dump(rec, open(a.out, "w"), indent=1)
        return
    import torch
    from wiggletools_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    ds, df = torch.from_numpy(s).to(dev), torch.from_numpy(f).to(dev)
    rec = {"tool": "tools/hist_time.py", "device": torch.cuda.get_device_name(0), "dataset_runs": n, "value": "f32", "reps": a.reps,
           "timing": "events around the call, pool allocations included; --reps after one warm-up per shape: ms lists every repeat, best_ms the minimum, "
                     "spread = (max - min) / min",
           "GB_per_s": "12 B per run / time (each of the two passes reads those bytes once)", "shapes": {}, "skewed_over_uniform": {}}
    ln = (f.astype(np.int64) - s.astype(np.int64))
    for kind, v in values.items():
        dv = torch.from_numpy(v).to(dev)
        dv64 = dv.double()
        runs = _lib.Runs(n, ds.data_ptr(), df.data_ptr(), dv64.data_ptr(), None)
        m6 = np.zeros(6)
        t = timed(a.reps, lambda: _lib.check(L.wtamd_runs_moments(C.byref(runs), n, m6.ctypes.data, None)))
        mom = {"ms": t, "best_ms": min(t), "median_ms": float(np.median(t)), "spread": (max(t) - min(t)) / min(t), "GB_per_s": 16.0 * n / (min(t) * 1e-3) / 1e9}
        rec["runs_moments_f64_" + kind] = mom
        print(json.dumps({"runs_moments_f64_" + kind: mom}), flush=True)
        del dv64
        for rows in ROWS:
            seg = np.linspace(0, n, rows + 1).astype(np.int64)
            row = np.arange(rows, dtype=np.int32)
            for w in widths:
                out = torch.empty((rows, w), dtype=torch.float64, device=dev)
                r2 = np.zeros(2)
                t = timed(a.reps, lambda: _lib.check(L.wtamd_runs_histogram(rows, seg.ctypes.data, row.ctypes.data, rows, ds.data_ptr(), df.data_ptr(),
                                                                            dv.data_ptr(), 0, w, 0, r2.ctypes.data, out.data_ptr(), None)))
                best = min(t) * 1e-3
                name = "%s_rows%d_w%d" % (kind, rows, w)
                d = {"values": kind, "rows": rows, "width": w, "regime": "LDS" if w <= lds_width else "global", "ms": t, "best_ms": min(t),
                     "median_ms": float(np.median(t)), "spread": (max(t) - min(t)) / min(t), "runs_per_s": n / best, "GB_per_s": 12.0 * n / best / 1e9,
                     "time_over_runs_moments": min(t) / mom["best_ms"], "range": r2.tolist()}
                if not a.no_check:
                    got = out.cpu().numpy()
                    col = M.columns(v.astype(np.float64), r2[0], r2[1], w)
                    exp = np.zeros((rows, w))
                    for r in range(rows):                   # (whole numbers below 2^53: the float sums are exact)
                        exp[r] = np.bincount(col[seg[r]:seg[r + 1]], weights=ln[seg[r]:seg[r + 1]].astype(np.float64), minlength=w)
                    d["equal_to_numpy_bit_for_bit"] = bool(M.same_bits(got, exp) and M.same_bits(r2, M.value_range(v.astype(np.float64))))
                rec["shapes"][name] = d
                print(json.dumps({name: d}), flush=True)
                del out
        del dv
    for rows in ROWS:
        for w in widths:
            rec["skewed_over_uniform"]["rows%d_w%d" % (rows, w)] = rec["shapes"]["skewed_rows%d_w%d" % (rows, w)]["best_ms"] / \
                rec["shapes"]["uniform_rows%d_w%d" % (rows, w)]["best_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps({"skewed_over_uniform": rec["skewed_over_uniform"]}), flush=True)


if __name__ == "__main__":
    main()
