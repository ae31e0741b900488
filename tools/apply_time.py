"""Times the apply door (csrc/wt_apply.hip, wtamd_runs_apply) on the GPU and wtamd_runs_moments over the same list in the same
process: a one-region apply does strictly more work than that call (a search, a clip, the covered length), so its ratio to it
is the figure to watch.

Input (one segment): the dataset tools/region_time.py builds -- 6 * 10^7 runs that do not overlap, f32 values, resident in HBM --
against 10^6 regions of 10 runs each, 10^4 regions of 5 000 runs each, and 1 region over everything, strict and with fill-in.
Every call is timed with events around the whole call (its pool allocations, its passes and the copies of its counters
included), --reps times after one warm-up; the minimum counts.  GB/s = 12 bytes per run under a region / time.

With --reference <the reference's sources> the compiled reference's ApplyMultiplexer is timed INSTEAD, on this host's CPU, on
one thread, through the driver of tests/golden/make_apply_golden.py (array children, all seven statistics, strict): over
the same dataset and the first --ref-regions regions of each shape, as regions per second.  It needs no GPU and adds its
figures to the file the device run wrote.

  python tools/apply_time.py [--out profiles/apply.json] [--reps 3] [--runs 60000000] [--reference PATH]
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

SHAPES = (("1e6_regions_of_10_runs", 1_000_000, 10), ("1e4_regions_of_5000_runs", 10_000, 5_000), ("1_region_over_everything", 1, 0))


def make_regions(rng, s, f, count, runs):
    if runs == 0:
        return np.array([0], np.int32), np.array([int(f[-1])], np.int32)
    a = np.sort(rng.integers(0, len(s) - runs, count))
    return s[a].copy(), f[a + runs - 1].copy()


def reference(a, s, f, v, shapes):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_apply_golden as G
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        L = G.build(a.reference, tmp)
        for name, rs, rf, runs in shapes:
            k = min(len(rs), a.ref_regions if runs == 10 else max(a.ref_regions // 100, 1) if runs else 1)
            data = (["chr1"], [(s, f)], v.astype(np.float64))
            t0 = time.perf_counter()
            rec = G.run(L, ["chr1"], data, (["chr1"], [(rs[:k], rf[:k])]), 0.0, True, list(range(7)))
            dt = time.perf_counter() - t0
            out[name] = {"regions": k, "seconds": dt, "regions_per_s": k / dt, "runs_under_regions_per_s": k * (runs if runs else len(s)) / dt,
                         "AUC_first": rec["AUC"][0]}
            print(json.dumps({"reference": {name: out[name]}}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "apply.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--runs", type=int, default=60_000_000)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--ref-regions", type=int, default=20_000)
    a = ap.parse_args()
    rng = np.random.default_rng(2026)
    s, f, v = make_source(rng, a.runs)
    n = len(s)
    shapes = []
    for name, count, runs in SHAPES:
        rs, rf = make_regions(rng, s, f, count, runs)
        shapes.append((name, rs, rf, runs))
    if a.reference:
        rec = json.load(open(a.out)) if os.path.exists(a.out) else {"tool": "tools/apply_time.py"}
        rec["reference_1_thread"] = {"what": "the compiled reference's ApplyMultiplexer, seven statistics, strict, array children; on the CPU of the host "
                                             "that ran --reference (not the GPU host); a prefix of the regions of each shape: device_over_reference_regions_per_s is a "
                                             "ratio of rates EXTRAPOLATED from that prefix, not of like-for-like times",
                                     "shapes": reference(a, s, f, v, shapes)}
        for name, d in rec["reference_1_thread"]["shapes"].items():
            if name in rec and "strict" in rec[name]:
                rec[name]["device_over_reference_regions_per_s"] = rec[name]["strict"]["regions_per_s"] / d["regions_per_s"]
        json.dump(rec, open(a.out, "w"), indent=1)
        return
    import torch
    from wiggletools_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    ds, df, dv = torch.from_numpy(s).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(v).to(dev)
    dv64 = dv.double()
    seg = np.array([0, n], np.int64)
    rec = {"tool": "tools/apply_time.py", "device": torch.cuda.get_device_name(0), "dataset_runs": n, "span_bp": int(f[-1]), "value": "f32",
           "timing": "events around the call, pool allocations included; minimum of --reps after one warm-up",
           "GB_per_s": "12 B per run under a region / time"}
    runs = _lib.Runs(n, ds.data_ptr(), df.data_ptr(), dv64.data_ptr(), None)
    m6 = np.zeros(6)
    t = timed(a.reps, lambda: _lib.check(L.wtamd_runs_moments(C.byref(runs), n, m6.ctypes.data, None)))
    rec["runs_moments_f64"] = {"ms": t, "best_ms": min(t), "GB_per_s": 16.0 * n / (min(t) * 1e-3) / 1e9, "moments6": m6.tolist()}
    print(json.dumps({"runs_moments_f64": rec["runs_moments_f64"]}), flush=True)
    for name, rs, rf, per in shapes:
        drs, drf = torch.from_numpy(rs).to(dev), torch.from_numpy(rf).to(dev)
        rseg = np.array([0, len(rs)], np.int64)
        out = torch.empty((len(rs), 6), dtype=torch.float64, device=dev)
        under = len(rs) * per if per else n
        r = {"regions": len(rs), "runs_under_regions": under}
        for mode, flags in (("strict", 1), ("fillin", 0)):
            t = timed(a.reps, lambda: _lib.check(L.wtamd_runs_apply(1, seg.ctypes.data, ds.data_ptr(), df.data_ptr(), dv.data_ptr(), 0, rseg.ctypes.data,
                                                                    drs.data_ptr(), drf.data_ptr(), 0.0, flags, out.data_ptr(), None)))
            best = min(t) * 1e-3
            r[mode] = {"ms": t, "best_ms": min(t), "regions_per_s": len(rs) / best, "GB_per_s": 12.0 * under / best / 1e9,
                       "time_over_runs_moments": min(t) / rec["runs_moments_f64"]["best_ms"], "first_region_moments6": out[0].cpu().tolist()}
        if not per:                       # the same list through both doors: the same span and extremes, the sums to rounding
            got, ref = r["strict"]["first_region_moments6"], rec["runs_moments_f64"]["moments6"]
            assert got[1] == ref[1] and got[3] == ref[3] and got[4] == ref[4] and abs(got[0] - ref[0]) <= 1e-9 * abs(ref[0]) + 1e-6, (got, ref)
            assert abs(got[2] - ref[2]) <= 1e-9 * ref[2], (got, ref)
        rec[name] = r
        print(json.dumps({name: r}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
