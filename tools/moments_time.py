"""Measurements of the run-moments path (csrc/wt_moments.hip), on the GPU.

  --kernels   the resident output run list of `mean` over one large chromosome of 100 synthetic tracks (the bench's
              generator), then wtamd_runs_auc and wtamd_runs_moments over it, --reps times each.  Run it under
              `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/moments_time.py --kernels`
              (a run of its own, no counters) and take the KERNEL durations from DIR's *kernel_stats.csv with
  --summary CSV --runs N   -> one JSON line: average ns of wt_auc_kernel and wt_moments_kernel (+ their final kernels),
              their ratio, and the fraction of the HBM peak that 16 bytes per run over those times amount to.
  --e2e       `varI mean` over 100 synthetic tracks through wtamd_VarianceIntegrator (tests/integ_driver.c, children popped
              one interval at a time), fused against WTAMD_NO_FUSED_INTEGRATORS=1: bp/s and bytes device -> host.
  --accuracy  T of the device against the reference's sequential update and a long-double sum, as mean / deviation grows.
"""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12       # bytes / s, MI355X


def _tracks(clen, mean_run):
    import torch
    from wiggletools_amd import engine, synthgen
    torch.cuda.set_device(0)
    seg, s, f, v = synthgen.device_tracks(2024, [clen], 100, mean_run=mean_run)
    return engine.TrackSet.from_device(1, 100, seg, s, f, v, np.zeros(100)), (seg, s, f, v)


def kernels(args):
    import torch
    ts, _ = _tracks(args.bp, 16.0)
    out = ts.alloc_runs()
    n = ts.reduce("mean", out)
    for _ in range(args.reps):
        a = out.auc()
        m = out.moments()
    torch.cuda.synchronize()
    print(json.dumps({"runs": n, "bp": args.bp, "auc": a, "moments": m.tolist()}))


def summary(args):
    rows = list(csv.DictReader(open(args.summary)))
    def avg(key):
        r = [x for x in rows if key in x["Name"]]
        return float(r[0]["AverageNs"]) if r else float("nan")
    auc, auc_f = avg("wt_auc_kernel"), avg("wt_auc_final_kernel")
    mom, mom_f = avg("wt_moments_kernel"), avg("wt_moments_final_kernel")
    b = 16.0 * args.runs
    print(json.dumps({"runs": args.runs, "wt_auc_kernel_ns": auc, "wt_auc_final_kernel_ns": auc_f, "wt_moments_kernel_ns": mom,
                      "wt_moments_final_kernel_ns": mom_f, "moments_over_auc": mom / auc,
                      "moments_with_final_over_auc_with_final": (mom + mom_f) / (auc + auc_f),
                      "auc_fraction_of_hbm_peak": b / (auc * 1e-9) / HBM_PEAK,
                      "moments_fraction_of_hbm_peak": b / (mom * 1e-9) / HBM_PEAK}))


def e2e(args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_integrator_moments as T
    from wiggletools_amd import _lib
    _, (seg, s, f, v) = _tracks(args.bp, 64.0)
    d = dict(n_chrom=1, n_tracks=100, seg_off=seg, start=s.cpu().numpy(), finish=f.cpu().numpy(), value=v.double().cpu().numpy(),
             defaults=np.zeros(100))
    bp = int(d["finish"].max() - d["start"].min())
    D = T.Driver(T._driver_lib(tempfile.mkdtemp()), _lib.LIB_PATH, "wtamd_")
    rec = {"bp": bp, "tracks": 100, "intervals": int(seg[-1])}
    for tag, env in (("fused", None), ("host", "1"), ("fused_again", None)):
        if env:
            os.environ["WTAMD_NO_FUSED_INTEGRATORS"] = env
        else:
            os.environ.pop("WTAMD_NO_FUSED_INTEGRATORS", None)
        t0 = time.perf_counter()
        got, pops, d2h, runs = D.run(d, "var", "mean", 0)
        dt = time.perf_counter() - t0
        rec[tag] = {"varI": got, "pops": pops, "d2h_bytes": d2h, "runs": runs, "seconds": dt, "bp_per_s": bp / dt}
    print(json.dumps(rec))


def accuracy(args):
    """T of 2e6 runs of full-mantissa values, mean `m` and deviation 1: the device's ordered merge and the reference's
    sequential update, each against a long-double two-pass sum."""
    import torch
    from wiggletools_amd.engine import DeviceRuns
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_integrator_moments import _sequential
    rng = np.random.default_rng(5)
    n = 2_000_000
    length = rng.integers(1, 40, n)
    finish = np.cumsum(length).astype(np.int32) + 1
    start = (finish - length).astype(np.int32)
    rec = {"runs": n}
    for m in (50.0, 1e4, 1e6):
        v = rng.normal(m, 1.0, n)
        w, x = length.astype(np.longdouble), v.astype(np.longdouble)
        mean = (w * x).sum() / w.sum()
        exact = float((w * (x - mean) ** 2).sum())
        dev = torch.device("cuda", 0)
        r = DeviceRuns(torch.from_numpy(start).to(dev), torch.from_numpy(finish).to(dev), torch.from_numpy(v).to(dev),
                       torch.zeros(2, dtype=torch.int64, device=dev))
        T_dev = float(r.moments(n)[2])
        T_seq = _sequential(start, finish, v)[0]
        rec["mean_%g" % m] = {"device_vs_exact": abs(T_dev - exact) / exact, "sequential_vs_exact": abs(T_seq - exact) / exact,
                             "device_vs_sequential": abs(T_dev - T_seq) / exact}
    print(json.dumps(rec))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--summary", default=None)
    ap.add_argument("--runs", type=int, default=0)
    ap.add_argument("--bp", type=int, default=60_000_000)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if a.kernels:
        kernels(a)
    elif a.e2e:
        e2e(a)
    elif a.accuracy:
        accuracy(a)
    elif a.summary:
        summary(a)
